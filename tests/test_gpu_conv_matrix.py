"""yv3_conv2d launch path x descriptor feature, against one float64 restatement of the descriptor (tests/conv_ref.py).

Every descriptor is built here directly (ctypes yv3_conv_desc), so that features the engine never combines -- alpha == NULL in a plane
mode, forced tiles with cin_up, fused decode with y == NULL, batch slices -- run too.  Every output buffer is NaN-filled with a NaN canary
behind it; after each launch: every output element written, nothing past the end, status word 0 (unless the case saturates on purpose),
and the result within the mode's bar of the reference -- 2e-5 * max(1,|ref|) for F32 / F32X3 / F32H2 and for the fp32 head outputs of a
BF16 conv; for the bf16 outputs of BF16, against a reference fed the bf16-rounded operands, ONE bf16 rounding of float64 plus the fp32
summation round-off (conv_ref.assert_bf16: criteria A and B), next to the old 2e-2 * max(1,|ref|).  Where the code documents the same K
order (the F32 tiles among themselves, the plane tile codes among themselves) the forced paths must also equal the library's default
choice bit for bit.  Shapes with hundreds of 128-row blocks are compared on conv_ref.sample_rows only."""
import ctypes
import types

import pytest
import torch

from yolo_v3_amd import _ffi, engine
from tests import conv_ref as cr

pytestmark = pytest.mark.gpu

F32, BF16, F32X3, F32H2 = _ffi.F32, _ffi.BF16, _ffi.F32X3, _ffi.F32H2
EINVAL, ESHAPE, EDTYPE = -1, -2, -4
BAR = {F32: 2e-5, F32X3: 2e-5, F32H2: 2e-5, BF16: 2e-2}
CANARY = 4096                       # NaN elements behind every output buffer
FP16_MAX = 65504.0
NAN = float("nan")
TILE_SHIFT = 8                      # YV3_OPT_TILE_SHIFT (include/yv3.h): forced tile code of the plane kernels


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    yield
    torch.cuda.synchronize()


def _lib():
    return _ffi.lib()


def _tile(code):
    return (code & 0xff) << TILE_SHIFT


def _rand(shape, g, lo=-1.0, hi=1.0):
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def _held(t_nhwc, mode):
    """(device tensor in the operand format of `mode`, the fp32 values it holds on the host)."""
    dev = engine.to_planes(t_nhwc.cuda(), mode)
    return dev, engine.from_planes(dev, mode).cpu()


def _ptr(t):
    return t.data_ptr() if t is not None else None


class Conv:
    """One convolution's operands on the device and on the host.  Weights are uniform in [-1, 1] and packed unscaled through
    yv3_pack_conv_weight; alpha (when not None) carries the 1/sqrt(fan-in) scale."""

    def __init__(self, mode, cin, cout, k=1, stride=1, B=1, H=8, W=8, res=False, cin_up=0, alpha_none=False, out_f32=False,
                 cout_pad=None, act=cr.ACT_LEAKY, seed=0):
        self.mode, self.cin, self.cout, self.k, self.stride = mode, cin, cout, k, stride
        self.B, self.H, self.W, self.cin_up, self.act = B, H, W, cin_up, act
        self.out_dtype = F32 if out_f32 else mode
        self.cout_pad = cout_pad if cout_pad is not None else (cout + 31) // 32 * 32
        self.Ho, self.Wo = cr.out_hw(H, W, k, stride)
        self.M = B * self.Ho * self.Wo
        self._mag = None                # (pixels, conv_ref.conv_desc_mag on them): the BF16 bar's magnitude, computed once per row set
        g = torch.Generator().manual_seed(1000 + seed)
        if cin_up:
            self.x, self.x_ref = _held(_rand((B, H // 2, W // 2, cin_up), g), mode)
            self.x2, self.x2_ref = _held(_rand((B, H, W, cin - cin_up), g), mode)
        else:
            self.x, self.x_ref = _held(_rand((B, H, W, cin), g), mode)
            self.x2 = self.x2_ref = None
        w = _rand((cout, cin, k, k), g)
        self.w_ref = w.bfloat16().float() if mode == BF16 else w
        np_ = engine.PLANES[mode]
        n = self.cout_pad * k * k * cin
        self.w_oihw = w.cuda()
        self.wp = torch.empty(max(1, np_) * n, device="cuda", dtype=engine._TORCH_DTYPE[mode])
        _ffi.check(_lib().yv3_pack_conv_weight(self.w_oihw.data_ptr(), self.wp.data_ptr(), cout, cin, k, self.cout_pad, mode,
                                                _ffi.stream_ptr()), "yv3_pack_conv_weight")
        self.alpha_ref = None if alpha_none else (_rand((cout,), g, 0.5, 1.5) / (cin * k * k) ** 0.5)
        self.beta_ref = _rand((cout,), g, -0.2, 0.2)
        self.alpha = self.alpha_ref.cuda() if self.alpha_ref is not None else None
        self.beta = self.beta_ref.cuda()
        self.res = self.res_ref = None
        if res:
            self.set_residual(_rand((B, self.Ho, self.Wo, cout), g, -0.5, 0.5))
        self.flags = torch.zeros(1, dtype=torch.int32, device="cuda")

    def set_residual(self, r_nhwc):
        self.res, self.res_ref = _held(r_nhwc, self.mode)
        self._mag = None

    def set_beta(self, beta):
        self._mag = None
        self.beta_ref = beta.clone()
        self.beta = beta.cuda()

    def y_elems(self):
        return self.M * self.cout * (1 if self.out_dtype == F32 else engine.PLANES[self.mode])

    def new_y(self):
        dt = torch.float32 if self.out_dtype == F32 else engine._TORCH_DTYPE[self.mode]
        return torch.full((self.y_elems() + CANARY,), NAN, dtype=dt, device="cuda")

    def desc(self, y, options=0, tune0=0, workspace=None):
        d = _ffi.ConvDesc()
        d.x, d.x2, d.w = _ptr(self.x), _ptr(self.x2), self.wp.data_ptr()
        d.alpha, d.beta, d.residual, d.y = _ptr(self.alpha), self.beta.data_ptr(), _ptr(self.res), _ptr(y)
        d.B, d.H, d.W, d.cin, d.cin_up = self.B, self.H, self.W, self.cin, self.cin_up
        d.cout, d.cout_pad, d.k, d.stride, d.act = self.cout, self.cout_pad, self.k, self.stride, self.act
        d.dtype, d.out_dtype, d.flags = self.mode, self.out_dtype, self.flags.data_ptr()
        if workspace is not None:
            d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel()
        d.options, d.tune[0] = options, tune0
        return d

    def launch(self, options=0, tune0=0, workspace=None, y=None):
        y = self.new_y() if y is None else y
        d = self.desc(y, options, tune0, workspace)
        _ffi.check(_lib().yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), "yv3_conv2d")
        return y

    def read(self, y):
        """[M, cout] fp32 values of an output buffer."""
        n = self.M * self.cout
        if self.out_dtype == F32:
            return y[:n].view(self.M, self.cout).cpu()
        np_ = engine.PLANES[self.mode]
        return engine.from_planes(y[:np_ * n].view(np_, self.M, self.cout), self.mode).cpu()

    def ref(self, pixels=None):
        return cr.conv_desc_ref(self.x_ref, self.w_ref, self.beta_ref, self.alpha_ref, self.res_ref, self.x2_ref, self.cin_up,
                                self.stride, self.act, pixels)

    def mag(self, pixels=None):
        """|alpha| * sum|w||x| + |beta| + |residual| of the same rows as ref(pixels)."""
        if self._mag is None or self._mag[0] is not pixels:
            self._mag = (pixels, cr.conv_desc_mag(self.x_ref, self.w_ref, self.beta_ref, self.alpha_ref, self.res_ref, self.x2_ref,
                                                  self.cin_up, self.stride, pixels))
        return self._mag[1]

    def check(self, y, ref, pixels=None, what="", flag=0):
        """Canary intact, every element written, status word == flag, values within the bar (on `pixels` only, if given).  BF16: the
        old 2e-2 bar AND conv_ref's -- A + B for a bf16 output, 2e-5 * max(1,|ref|) for an fp32 one."""
        torch.cuda.synchronize()
        n = self.y_elems()
        assert bool(torch.isnan(y[n:]).all()), "%s: wrote past the end of y" % what
        written = ~torch.isnan(y[:n])
        assert bool(written.all()), "%s: %d output elements not written" % (what, int((~written).sum()))
        assert int(self.flags.item()) == flag, "%s: status word %d" % (what, int(self.flags.item()))
        self.flags.zero_()
        got = self.read(y).double()
        if pixels is not None:
            got = got[pixels]
        err = (got - ref).abs() / ref.abs().clamp(min=1.0)
        bar = BAR[self.mode]
        assert float(err.max()) <= bar, "%s: max normalised error %.3g > %.1g at row/channel %s" % (
            what, float(err.max()), bar, divmod(int(err.argmax()), self.cout))
        if self.mode == BF16 and self.out_dtype == F32:
            e = cr.assert_f32_bar(got, ref, what)
            print("bf16 bar | %s | fp32 out | max normalised error %.3g" % (what, e))
        elif self.mode == BF16:
            r = cr.assert_bf16(got, ref, self.mag(pixels), self.k * self.k * self.cin, what)
            print("bf16 bar | %s | worst |d|/eps %.4g | share %.3g" % (what, r["worst"], r["share"]))
        return got


def _run_paths(conv, paths, bitwise, pixels=None, what=""):
    """Launch `conv` along every (name, options, tune0, workspace) path; check each against the reference, and the names in `bitwise`
    against the first path bit for bit."""
    ref = conv.ref(pixels)
    outs = {}
    for name, options, tune0, ws in paths:
        y = conv.launch(options, tune0, ws)
        conv.check(y, ref, pixels, "%s [%s]" % (what, name))
        outs[name] = y
    first = paths[0][0]
    n = conv.y_elems()
    for name in bitwise:
        assert torch.equal(outs[name][:n], outs[first][:n]), "%s: path %s differs from %s" % (what, name, first)
    return outs


# ----------------------------------------------------------------------------- exact fp32 (conv_igemm_f32.hip)
LANES = ("two lanes", _ffi.OPT_TWO_LANES, 0, None)        # the unpinned instantiation of the same tile

# name, cin, cout, cout_pad, k, stride, B, H, W, residual, cin_up, head
F32_SMALL = [
    ("64x64 1x1 res", 64, 128, 128, 1, 1, 3, 13, 15, True, 0, False),
    ("64x64 k3s1 res", 64, 128, 128, 3, 1, 2, 13, 11, True, 0, False),
    ("64x64 k3s2", 32, 128, 128, 3, 2, 2, 15, 13, False, 0, False),
    ("64x64 up32 res", 96, 128, 128, 1, 1, 3, 14, 10, True, 32, False),
    ("64x64 up128", 160, 128, 128, 1, 1, 2, 10, 6, False, 128, False),
    ("64x64 head255", 128, 255, 256, 1, 1, 2, 13, 13, False, 0, True),
    ("128x64 1x1 res", 64, 64, 64, 1, 1, 3, 13, 15, True, 0, False),
    ("128x64 k3s1 res", 32, 64, 64, 3, 1, 2, 11, 13, True, 0, False),
    ("128x64 k3s2 res", 64, 192, 192, 3, 2, 2, 15, 13, True, 0, False),
    ("128x64 up32", 96, 192, 192, 1, 1, 2, 14, 10, False, 32, False),
    ("128x32 1x1 res", 64, 32, 32, 1, 1, 3, 13, 15, True, 0, False),
    ("128x32 k3s1 res", 64, 96, 96, 3, 1, 2, 11, 13, True, 0, False),
    ("128x32 k3s2", 32, 160, 160, 3, 2, 2, 15, 13, False, 0, False),
    ("128x32 up128 res", 192, 96, 96, 1, 1, 2, 10, 14, True, 128, False),
    ("128x32 head18", 128, 18, 32, 1, 1, 2, 13, 13, False, 0, True),
    ("128x32 head75", 128, 75, 96, 1, 1, 2, 13, 13, False, 0, True),
]


def _f32_conv(cin, cout, cout_pad, k, s, B, H, W, res, cin_up, head, seed):
    return Conv(F32, cin, cout, k, s, B, H, W, res=res, cin_up=cin_up, alpha_none=head, cout_pad=cout_pad,
                act=cr.ACT_LINEAR if head else cr.ACT_LEAKY, seed=seed)


@pytest.mark.parametrize("case", F32_SMALL, ids=[c[0] for c in F32_SMALL])
def test_f32_tiles_small_vs_fp64(case):
    """64x64 (cout_pad % 128 == 0, few blocks; also forced by tune[0] = 2), 128x64 (cout 64 / 192) and 128x32 (cout_pad 32 / 96 / 160)
    tiles: 1x1, 3x3 s1 and s2 on odd pictures, residual, cin_up 32 / 128 with B > 1 and odd W/2, plain alpha == NULL heads;
    the unpinned instantiation (YV3_OPT_TWO_LANES) equals the pinned one bit for bit."""
    name = case[0]
    conv = _f32_conv(*case[1:], seed=len(name))
    paths = [("default", 0, 0, None), LANES] + ([("tune0=2", 0, 2, None)] if case[3] % 128 == 0 else [])
    _run_paths(conv, paths, [p[0] for p in paths[1:]], what=name)


# big shapes: >= 384 blocks of 128 rows, so the 128x128 rules apply; compared on the sampled rows
F32_BIG = [
    # 3x3 s2 on an odd picture: 37 x 26 x 27 = 25974 rows, 406 blocks -- the eight-wave 128x128 tile by the rule
    ("k3s2 res", (128, 256, 256, 3, 2, 37, 51, 53, True, 0, False),
     [("default", 0, 0, None), ("four waves", 0, 6, None), ("64x64", 0, 2, None), LANES]),
    ("k3s1", (64, 256, 256, 3, 1, 37, 26, 26, False, 0, False),
     [("default", 0, 0, None), ("four waves", 0, 6, None), ("64x64", 0, 2, None)]),
    # 1x1 with a residual (the persistent GEMM declines it): 64x64 by default, 128x128 with tune[0] = 7 (eight waves) / 6 (four)
    ("1x1 res", (512, 256, 256, 1, 1, 37, 26, 26, True, 0, False),
     [("eight waves", 0, 7, None), ("default", 0, 0, None), ("four waves", 0, 6, None), ("two lanes", _ffi.OPT_TWO_LANES, 7, None)]),
    ("1x1 up128", (384, 256, 256, 1, 1, 37, 26, 26, False, 128, False),
     [("eight waves", 0, 7, None), ("default", 0, 0, None), ("four waves", 0, 6, None)]),
    ("head255", (256, 255, 256, 1, 1, 37, 26, 26, False, 0, True),
     [("eight waves", 0, 7, None), ("default", 0, 0, None), ("four waves", 0, 6, None), ("two lanes", _ffi.OPT_TWO_LANES, 7, None)]),
]


@pytest.mark.parametrize("name,shape,paths", F32_BIG, ids=[c[0] for c in F32_BIG])
def test_f32_tiles_big_vs_fp64_sampled(name, shape, paths):
    """The 128x128 eight-wave tile (3x3 by the rule; 1x1 layers the GEMM declines with tune[0] = 7), the four-wave 128x128 tile
    (tune[0] = 6) and 64x64 (tune[0] = 2 / the 1x1 default) on launches of >= 384 blocks: same K order, same bits; against fp64 on the
    sampled rows (every border of image 0, first / last pixel of every image, the last tile, 2048 random rows)."""
    conv = _f32_conv(*shape, seed=len(name) + 50)
    rows = cr.sample_rows(conv.B, conv.Ho, conv.Wo, seed=3)
    _run_paths(conv, paths, [p[0] for p in paths[1:]], pixels=rows, what=name)


# ----------------------------------------------------------------------------- plane modes (conv_planes.hip, _w4, _k3s1)
PLANE_CODES = {F32X3: (1, 2), F32H2: (1, 2, 3, 12), BF16: (7, 8, 11, 13, 14, 15, 16)}

# name, kwargs of Conv
PLANE_CASES = [
    ("k3s1 res", dict(cin=128, cout=256, k=3, stride=1, B=3, H=13, W=11, res=True)),
    ("k3s2 res", dict(cin=64, cout=128, k=3, stride=2, B=2, H=27, W=25, res=True)),
    ("1x1 res", dict(cin=256, cout=128, k=1, B=5, H=9, W=7, res=True)),
    ("up128 res", dict(cin=192, cout=256, k=1, B=3, H=10, W=14, res=True, cin_up=128)),
    ("up32", dict(cin=96, cout=128, k=1, B=2, H=6, W=10, cin_up=32)),
    ("alpha NULL k3 res", dict(cin=64, cout=128, k=3, stride=1, B=2, H=9, W=11, res=True, alpha_none=True)),
    ("alpha NULL 1x1", dict(cin=128, cout=256, k=1, B=2, H=7, W=9, alpha_none=True)),
    ("head18", dict(cin=128, cout=18, cout_pad=32, B=2, H=13, W=13, alpha_none=True, out_f32=True, act=cr.ACT_LINEAR)),
    ("head75", dict(cin=128, cout=75, cout_pad=96, B=2, H=13, W=13, alpha_none=True, out_f32=True, act=cr.ACT_LINEAR)),
    ("head255", dict(cin=256, cout=255, cout_pad=256, B=3, H=13, W=13, alpha_none=True, out_f32=True, act=cr.ACT_LINEAR)),
    ("one image < one tile", dict(cin=128, cout=256, k=3, stride=1, B=1, H=7, W=9, res=True)),
]


@pytest.mark.parametrize("mode", [F32X3, F32H2, BF16], ids=["F32X3", "F32H2", "BF16"])
@pytest.mark.parametrize("name,kw", PLANE_CASES, ids=[c[0] for c in PLANE_CASES])
def test_plane_paths_vs_fp64(mode, name, kw):
    """Default choice and every forced tile code of the mode (F32H2 1, 2, 3, 12; BF16 7, 8, 11, 13-16; F32X3 1, 2) bit for bit equal
    to each other -- a code the descriptor's features make the library decline must still give the default's result -- plus, in F32H2,
    the stream-K workspace and YV3_OPT_K3S1 (other summation orders: bar only).  Residual, cin_up, alpha == NULL, fp32 head outputs,
    M tails down to one image smaller than one tile."""
    conv = Conv(mode, seed=len(name) * 7 + mode, **kw)
    paths = [("default", 0, 0, None)] + [("code %d" % c, _tile(c), 0, None) for c in PLANE_CODES[mode]]
    bitwise = [p[0] for p in paths[1:]]
    if mode == F32H2:
        ws = torch.zeros(_lib().yv3_conv_workspace_bytes(), dtype=torch.uint8, device="cuda")
        paths.append(("stream-K", 0, 0, ws))
        if conv.k == 3:
            paths.append(("k3s1", _ffi.OPT_K3S1, 0, None))
    _run_paths(conv, paths, bitwise, what="%s mode %d" % (name, mode))
    if mode == F32H2:
        assert int(ws[-4 * 512:].view(torch.int32).abs().sum()) == 0          # every stream-K hand-over flag consumed


# ----------------------------------------------------------------------------- BF16: the tiles the rules pick on large launches
def _num_cu():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    return n & ~7 if n >= 8 else 256


def _cdiv(a, b):
    return -(-a // b)


def _bf16_tile_rule(M, cout_pad, k3, out_f32, ncu):
    """The tile yv3_conv2d_planes (conv_planes.hip) takes for a one-plane (BF16) descriptor with cout_pad % 128 == 0, no forced code
    and no tune bits, and the tile counts the rule looks at."""
    assert cout_pad % 128 == 0
    blocks256 = _cdiv(M, 256) * (cout_pad // 128)
    counts = {"blocks256": blocks256}
    if k3 and not out_f32 and cout_pad % 256 == 0:
        t256, t192 = _cdiv(M, 256) * (cout_pad // 256), _cdiv(M, 192) * (cout_pad // 256)
        r256, r192 = _cdiv(t256, ncu) * ncu, _cdiv(t192, ncu) * ncu
        counts.update(t256=t256, t192=t192)
        if t192 * 100 >= 85 * r192 and t256 * 100 < 80 * r256:
            return "192x256 ping-pong", counts
        if (t256 * 10 >= 6 * ncu) if t256 <= ncu else (t256 * 10 >= 8 * r256):
            return "256x256 ping-pong", counts
    if blocks256 >= 256 and not out_f32:
        return ("256x128 four waves, rolling" if k3 else "256x128 four waves, plain"), counts
    if blocks256 >= 128:
        return "256x128 eight waves, 6-deep", counts
    return "128x128", counts


# name, the tile the rule must pick, Conv kwargs without B: the smallest B at which the rule picks that tile is searched at run time from
# the device's CU count (on 256 CUs: 58, 62, 7, 25, 96, 96)
BF16_RULE_CASES = [
    ("i 128-1024 k3 @13", "256x256 ping-pong", dict(cin=128, cout=1024, k=3, H=13, W=13, res=True)),
    ("ii 512-1024 k3 @13", "192x256 ping-pong", dict(cin=512, cout=1024, k=3, H=13, W=13)),
    ("iii 64-128 k3 @104", "256x128 four waves, rolling", dict(cin=64, cout=128, k=3, H=104, W=104, res=True)),
    ("iv 256-128 1x1 @52", "256x128 four waves, plain", dict(cin=256, cout=128, k=1, H=52, W=52)),
    ("v 512-256 1x1 @13", "256x128 eight waves, 6-deep", dict(cin=512, cout=256, k=1, H=13, W=13, res=True)),
    ("v head255 @13", "256x128 eight waves, 6-deep", dict(cin=256, cout=255, cout_pad=256, k=1, H=13, W=13, alpha_none=True, out_f32=True,
                                                          act=cr.ACT_LINEAR)),
]


# _bf16_tile_rule's names -> the kernel and the loop yv3_conv2d_kernel names (csrc/conv_select.h: YV3_PK_* without the prefix, yv3_planes_loop)
BF16_RULE_KERNEL = {"256x256 ping-pong": "256x256_PP4", "192x256 ping-pong": "192x256_PP4", "256x128 four waves, rolling": "256x128_W4_ROLL",
                    "256x128 four waves, plain": "256x128_W4", "256x128 eight waves, 6-deep": "256x128_W8_PP6", "128x128": "128x128_W8"}
BF16_RULE_LOOP = {"256x256 ping-pong": "pingpong", "192x256 ping-pong": "pingpong", "256x128 four waves, rolling": "rolling",
                  "256x128 four waves, plain": "plain", "256x128 eight waves, 6-deep": "pingpong", "128x128": "plain"}


@pytest.mark.parametrize("name,tile,kw", BF16_RULE_CASES, ids=[c[0] for c in BF16_RULE_CASES])
def test_bf16_rule_tiles_vs_fp64_sampled(name, tile, kw):
    """The BF16 tiles that only large launches reach -- 256x256 and 192x256 ping-pong, the four-wave 256x128 tile with the rolling (3x3)
    and the plain (1x1) loop, the eight-wave 6-deep 256x128 tile (a 1x1 layer and an fp32 head) -- each at the smallest batch at which
    the selection rule picks it on this device, against float64 on conv_ref.sample_rows with the BF16 bar (A + B; the head: the fp32
    bar), and bit for bit against forced code 7 (the four-wave rolling tile: same K order)."""
    ncu = _num_cu()
    cout_pad = kw.get("cout_pad", kw["cout"])
    Ho, Wo = cr.out_hw(kw["H"], kw["W"], kw["k"], 1)
    rule = lambda b: _bf16_tile_rule(b * Ho * Wo, cout_pad, kw["k"] == 3, kw.get("out_f32", False), ncu)
    B = next((b for b in range(1, 513) if rule(b)[0] == tile), None)
    assert B is not None, "%s: no batch up to 512 makes the rule pick the %s tile on %d CUs" % (name, tile, ncu)
    picked, counts = rule(B)
    print("bf16 rule | %s | %d CUs | B = %d | %s | %s" % (name, ncu, B, picked, counts))
    # the tile counts this case relies on
    if tile == "256x256 ping-pong":
        assert counts["t256"] * 10 >= 6 * ncu and counts["t256"] <= ncu
        assert not (counts["t192"] * 100 >= 85 * _cdiv(counts["t192"], ncu) * ncu and counts["t256"] * 100 < 80 * ncu)
    elif tile == "192x256 ping-pong":
        assert counts["t192"] * 100 >= 85 * _cdiv(counts["t192"], ncu) * ncu and counts["t256"] * 100 < 80 * _cdiv(counts["t256"], ncu) * ncu
    elif tile.startswith("256x128 four waves"):
        assert counts["blocks256"] >= 256 and cout_pad % 256 != 0
    else:
        assert 128 <= counts["blocks256"] and (kw.get("out_f32", False) or counts["blocks256"] < 256)
    conv = Conv(BF16, B=B, seed=300 + len(name), **kw)
    # ... and the library itself names that tile for the descriptor the "default" path launches (yv3_conv2d_kernel)
    line = _ffi.conv2d_kernel(conv.desc(None))
    print("bf16 rule | %s | yv3_conv2d_kernel: %s" % (name, line))
    assert line.split()[0] == BF16_RULE_KERNEL[tile] and line.split()[2] == BF16_RULE_LOOP[tile], (name, tile, line)
    rows = cr.sample_rows(conv.B, conv.Ho, conv.Wo, seed=5)
    _run_paths(conv, [("default", 0, 0, None), ("code 7", _tile(7), 0, None)], ["code 7"], pixels=rows, what=name)


# ----------------------------------------------------------------------------- fused decode
ANCHORS = (116.0, 90.0, 156.0, 198.0, 373.0, 326.0)


@pytest.mark.parametrize("mode", [F32X3, F32H2, BF16], ids=["F32X3", "F32H2", "BF16"])
@pytest.mark.parametrize("num_class,cout_pad", [(20, 96), (80, 256)])
def test_fused_decode_writes_exactly_its_rows(mode, num_class, cout_pad):
    """dec_out in the middle of a NaN-filled [B, N_total, 5+C] tensor with dec_out_batch_stride = N_total * (5+C): exactly this scale's
    rows are written, they equal yv3_decode of the logits of the same descriptor bit for bit, y == NULL gives the same bits, and the
    logits meet the mode's bar."""
    attrs = 5 + num_class
    B, H, W, before, after = 2, 13, 13, 37, 11
    rows = H * W * 3
    ntot = before + rows + after
    conv = Conv(mode, 128, 3 * attrs, 1, 1, B, H, W, alpha_none=True, out_f32=True, cout_pad=cout_pad, act=cr.ACT_LINEAR,
                seed=num_class + mode)
    lib = _lib()
    outs = []
    for bind_y in (True, False):
        dets = torch.full((B, ntot, attrs), NAN, device="cuda")
        y = conv.new_y()
        d = conv.desc(y if bind_y else None)
        d.dec_out = dets.data_ptr() + before * attrs * 4
        d.dec_out_batch_stride = ntot * attrs
        d.dec_stride = 32.0
        for i, a in enumerate(ANCHORS):
            d.dec_anchors[i] = a
        _ffi.check(lib.yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), "yv3_conv2d (fused decode)")
        torch.cuda.synchronize()
        assert int(conv.flags.item()) == 0
        assert bool(torch.isnan(dets[:, :before]).all()) and bool(torch.isnan(dets[:, before + rows:]).all()), "wrote outside its rows"
        assert not bool(torch.isnan(dets[:, before:before + rows]).any()), "a row of the scale was not written"
        if bind_y:
            conv.check(y, conv.ref(), what="head logits mode %d" % mode)
            logits = y
        else:
            assert bool(torch.isnan(y).all())
        outs.append(dets)
    sep = torch.full((B, ntot, attrs), NAN, device="cuda")
    an = (ctypes.c_float * 6)(*ANCHORS)
    _ffi.check(lib.yv3_decode(logits.data_ptr(), 3 * attrs, an, 32.0, sep.data_ptr() + before * attrs * 4, ntot * attrs, B, H, W,
                              num_class, _ffi.stream_ptr()), "yv3_decode")
    torch.cuda.synchronize()
    assert torch.equal(outs[0][:, before:before + rows], sep[:, before:before + rows])
    assert torch.equal(outs[1][:, before:before + rows], sep[:, before:before + rows])


# ----------------------------------------------------------------------------- batch slices
@pytest.mark.parametrize("mode", [F32X3, F32H2, BF16], ids=["F32X3", "F32H2", "BF16"])
def test_batch_slice_equals_full_batch_bitwise(mode):
    """A descriptor over images [b0, b0+Bs) of larger x / x2 / y / residual plane tensors (base pointers offset, *_plane_stride = the
    full tensors' plane strides), with cin_up and residual: rows outside the slice stay NaN, the slice equals the full-batch launch
    (no workspace) bit for bit (include/yv3.h)."""
    B, b0, Bs = 6, 2, 3
    conv = Conv(mode, 384, 256, 1, 1, B, 26, 26, res=True, cin_up=128, seed=40 + mode)
    full = conv.launch()
    conv.check(full, conv.ref(), what="full batch mode %d" % mode)
    np_ = engine.PLANES[mode]
    per_y = conv.Ho * conv.Wo * conv.cout
    per_x, per_x2 = 13 * 13 * 128, 26 * 26 * 256
    y = conv.new_y()
    d = conv.desc(y)
    es = y.element_size()
    d.x, d.x_plane_stride = conv.x.data_ptr() + b0 * per_x * es, B * per_x
    d.x2, d.x2_plane_stride = conv.x2.data_ptr() + b0 * per_x2 * es, B * per_x2
    d.y, d.y_plane_stride = y.data_ptr() + b0 * per_y * es, B * per_y
    d.residual = conv.res.data_ptr() + b0 * per_y * es
    d.B = Bs
    _ffi.check(_lib().yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), "yv3_conv2d (batch slice)")
    torch.cuda.synchronize()
    assert int(conv.flags.item()) == 0
    planes, fplanes = y[:np_ * B * per_y].view(np_, B, per_y), full[:np_ * B * per_y].view(np_, B, per_y)
    assert bool(torch.isnan(planes[:, :b0]).all()) and bool(torch.isnan(planes[:, b0 + Bs:]).all()) and bool(torch.isnan(y[np_ * B * per_y:]).all())
    assert torch.equal(planes[:, b0:b0 + Bs], fplanes[:, b0:b0 + Bs])


# ----------------------------------------------------------------------------- saturation contract of the fp16-plane mode
SAT_CHANNEL = 5


def _sat_conv(with_residual):
    # 3 x 26 x 26 x (64 -> 512): 16 Winograd tiles of 128 x 128 (enough for its even schedule), 64 direct 128x128 tiles (stream-K)
    return Conv(F32H2, 64, 512, 3, 1, 3, 26, 26, res=with_residual, seed=77)


def _sat_paths(conv):
    ws = torch.zeros(_lib().yv3_conv_workspace_bytes(), dtype=torch.uint8, device="cuda")
    ww, aw = engine.pack_wino(conv.w_oihw, conv.alpha if conv.alpha is not None else torch.ones(conv.cout, device="cuda"),
                              types.SimpleNamespace(cin=conv.cin, cout=conv.cout), conv.cout_pad, F32H2)
    wino_ws = torch.zeros(_lib().yv3_wino_workspace_bytes(conv.B, conv.H, conv.W, conv.cin), dtype=torch.uint8, device="cuda")
    wino = (ww, aw, wino_ws)
    return [("default", 0, None, None), ("code 1", _tile(1), None, None), ("code 2", _tile(2), None, None),
            ("code 3", _tile(3), None, None), ("code 12", _tile(12), None, None), ("k3s1", _ffi.OPT_K3S1, None, None),
            ("stream-K", 0, ws, None), ("winograd", _ffi.OPT_WINO_ALWAYS, None, wino),
            ("winograd even", _ffi.OPT_WINO_ALWAYS | _ffi.OPT_WINO_EVEN, None, wino)]


def _sat_launch(conv, options, ws, wino):
    y = conv.new_y()
    d = conv.desc(y, options, 0, ws)
    if wino is not None:
        d.w_wino, d.alpha_wino = wino[0].data_ptr(), wino[1].data_ptr()
        d.wino_ws, d.wino_ws_bytes = wino[2].data_ptr(), wino[2].numel()
        assert _lib().yv3_conv2d_form(ctypes.byref(d)) == 1
    _ffi.check(_lib().yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), "yv3_conv2d")
    return y


def _check_sat(conv, y, ref, clipped, what):
    """`clipped`: bool [M, cout] mask of the elements whose reference exceeds 65504 -- stored exactly as +65504, bit 0 set iff any;
    every other element within the bar."""
    flag = 1 if bool(clipped.any()) else 0
    torch.cuda.synchronize()
    n = conv.y_elems()
    assert bool(torch.isnan(y[n:]).all()) and not bool(torch.isnan(y[:n]).any()), what
    assert int(conv.flags.item()) == flag, "%s: status word %d, expected %d" % (what, int(conv.flags.item()), flag)
    conv.flags.zero_()
    got = conv.read(y).double()
    assert bool((got[clipped] == FP16_MAX).all()), "%s: clipped values %s" % (what, got[clipped].unique()[:8].tolist())
    err = ((got - ref).abs() / ref.abs().clamp(min=1.0))[~clipped]
    assert float(err.max()) <= BAR[F32H2], "%s: max normalised error %.3g" % (what, float(err.max()))


@pytest.mark.parametrize("case", ["a: just under", "b: one channel over", "c: one element over"])
def test_f16_planes_saturation_flag_every_conv2d_path(case):
    """F32H2 stores |value| > 65504 as +-65504 and ORs bit 0 into *flags: the engine's fall-back to F32X3 hangs on it.  Every plane
    path that can saturate -- direct default, tile codes 1 / 2 / 3 / 12, k3s1, Winograd F(2x2) tile and even schedules, stream-K --
    (a) keeps the bit clear with a channel peaking just under the limit, (b) sets it with a channel pushed over by beta = 7e4 and stores
    exactly +65504 there, (c) sets it when ONE element (last M tile, last real channel) goes over through residual 65504 + a positive
    conv output, and clips only that element."""
    conv = _sat_conv(case.startswith("c"))
    beta = conv.beta_ref.clone()
    if case.startswith("a"):
        beta[SAT_CHANNEL] = 64900.0
    elif case.startswith("b"):
        beta[SAT_CHANNEL] = 7.0e4
    else:
        beta[conv.cout - 1] = 10.0                                     # this channel's outputs are positive everywhere
        r = conv.res_ref.clone().view(-1, conv.cout)
        r[conv.M - 1, conv.cout - 1] = FP16_MAX
        conv.set_residual(r.view(conv.B, conv.Ho, conv.Wo, conv.cout))
    conv.set_beta(beta)
    ref = conv.ref()
    clipped = ref > FP16_MAX
    if case.startswith("a"):
        assert not bool(clipped.any()) and float(ref.max()) > 64800
    elif case.startswith("b"):
        assert bool(clipped[:, SAT_CHANNEL].all()) and int(clipped.sum()) == conv.M
    else:
        assert int(clipped.sum()) == 1 and bool(clipped[conv.M - 1, conv.cout - 1])
    for name, options, ws, wino in _sat_paths(conv):
        _check_sat(conv, _sat_launch(conv, options, ws, wino), ref, clipped, "%s, %s" % (case, name))


def _fp16_planes(t_nhwc):
    return engine.to_planes(t_nhwc.cuda(), F32H2)


@pytest.mark.parametrize("over", [False, True], ids=["just under", "one channel over"])
def test_f16_planes_saturation_flag_conv_front(over):
    """yv3_conv_front (feature.mlist.0 + .1 in one launch): beta1 of one channel just under 65504 keeps bit 0 clear, beta1 = 7e4
    sets it and stores exactly +65504 in that channel; everything else within the bar of the fp64 two-layer reference."""
    B, H, W = 1, 64, 64
    g = torch.Generator().manual_seed(11)
    x = torch.rand(B, 3, H, W, generator=g)
    w0, a0, b0 = _rand((32, 3, 3, 3), g, -0.3, 0.3), _rand((32,), g, 0.5, 1.5), _rand((32,), g, -0.2, 0.2)
    w1, a1, b1 = _rand((64, 32, 3, 3), g), _rand((64,), g, 0.5, 1.5) / 288 ** 0.5, _rand((64,), g, -0.2, 0.2)
    b1[SAT_CHANNEL] = 7.0e4 if over else 64900.0
    w1p = torch.empty(2 * 64 * 9 * 32, device="cuda", dtype=torch.float16)
    _ffi.check(_lib().yv3_pack_conv_weight(w1.cuda().data_ptr(), w1p.data_ptr(), 64, 32, 3, 64, F32H2, _ffi.stream_ptr()))
    w0t = w0.permute(1, 2, 3, 0).contiguous().cuda()
    dev = [t.cuda() for t in (x, a0, b0, a1, b1)]
    n = 2 * B * (H // 2) * (W // 2) * 64
    y = torch.full((n + CANARY,), NAN, dtype=torch.float16, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ffi.check(_lib().yv3_conv_front(dev[0].data_ptr(), w0t.data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), w1p.data_ptr(),
                                     dev[3].data_ptr(), dev[4].data_ptr(), y.data_ptr(), B, H, W, flags.data_ptr(), _ffi.stream_ptr()),
               "yv3_conv_front")
    mid = cr.conv_desc_ref(x.permute(0, 2, 3, 1), w0, b0, a0).view(B, H, W, 32)
    ref = cr.conv_desc_ref(mid, w1, b1, a1, stride=2)
    conv = types.SimpleNamespace(y_elems=lambda: n, flags=flags, cout=64,
                                 read=lambda t: engine.from_planes(t[:n].view(2, -1, 64), F32H2).cpu())
    _check_sat(conv, y, ref, ref > FP16_MAX, "yv3_conv_front over=%s" % over)


@pytest.mark.parametrize("over", [False, True], ids=["just under", "one channel over"])
def test_f16_planes_saturation_flag_res_block64(over):
    """yv3_res_block64 (feature.mlist.2: 1x1 64->32, 3x3 32->64, residual): the same two cases through beta2."""
    B, H, W = 2, 32, 48
    g = torch.Generator().manual_seed(12)
    x = _rand((B, H, W, 64), g)
    w1, a1, b1 = _rand((32, 64, 1, 1), g), _rand((32,), g, 0.5, 1.5) / 8.0, _rand((32,), g, -0.2, 0.2)
    w2, a2, b2 = _rand((64, 32, 3, 3), g), _rand((64,), g, 0.5, 1.5) / 288 ** 0.5, _rand((64,), g, -0.2, 0.2)
    b2[SAT_CHANNEL] = 7.0e4 if over else 64900.0
    packed = []
    for w, co, k in ((w1, 32, 1), (w2, 64, 3)):
        p = torch.empty(2 * co * k * k * w.shape[1], device="cuda", dtype=torch.float16)
        _ffi.check(_lib().yv3_pack_conv_weight(w.cuda().data_ptr(), p.data_ptr(), co, w.shape[1], k, co, F32H2, _ffi.stream_ptr()))
        packed.append(p)
    xp = _fp16_planes(x)
    x_held = engine.from_planes(xp, F32H2).cpu()
    dev = [t.cuda() for t in (a1, b1, a2, b2)]
    n = 2 * B * H * W * 64
    y = torch.full((n + CANARY,), NAN, dtype=torch.float16, device="cuda")
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ffi.check(_lib().yv3_res_block64(xp.data_ptr(), packed[0].data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), packed[1].data_ptr(),
                                      dev[2].data_ptr(), dev[3].data_ptr(), y.data_ptr(), B, H, W, flags.data_ptr(), _ffi.stream_ptr()),
               "yv3_res_block64")
    mid = cr.conv_desc_ref(x_held, w1, b1, a1).view(B, H, W, 32)
    ref = cr.conv_desc_ref(mid, w2, b2, a2, residual=x_held)
    conv = types.SimpleNamespace(y_elems=lambda: n, flags=flags, cout=64,
                                 read=lambda t: engine.from_planes(t[:n].view(2, -1, 64), F32H2).cpu())
    _check_sat(conv, y, ref, ref > FP16_MAX, "yv3_res_block64 over=%s" % over)


# ----------------------------------------------------------------------------- error contract of the conv C-ABI
def _mut(**fields):
    def f(d, bufs):
        for k, v in fields.items():
            setattr(d, k, bufs[v] if isinstance(v, str) else v)
    return f


# name, mutation, expected code per dtype (F32, planes); None: that dtype does not have this case
ERROR_CASES = [
    ("x NULL", _mut(x=None), EINVAL, EINVAL),
    ("w NULL", _mut(w=None), EINVAL, EINVAL),
    ("beta NULL", _mut(beta=None), EINVAL, EINVAL),
    ("y NULL, dec_out NULL", _mut(y=None), EINVAL, EINVAL),
    ("B = 0", _mut(B=0), EINVAL, EINVAL),
    ("H = -2", _mut(H=-2), EINVAL, EINVAL),
    ("W = 0", _mut(W=0), EINVAL, EINVAL),
    ("cin = 0", _mut(cin=0), EINVAL, EINVAL),
    ("cout = -64", _mut(cout=-64), EINVAL, EINVAL),
    ("k = 2", _mut(k=2), ESHAPE, ESHAPE),
    ("stride 3", _mut(k=3, stride=3), ESHAPE, ESHAPE),
    ("1x1 stride 2", _mut(stride=2), ESHAPE, ESHAPE),
    ("cin % 32", _mut(cin=48), ESHAPE, ESHAPE),
    ("cout_pad < cout", _mut(cout=96), ESHAPE, ESHAPE),
    ("cout_pad % 32", _mut(cout_pad=80), ESHAPE, ESHAPE),
    ("cin_up with k = 3", _mut(cin_up=32, x2="x2", k=3), ESHAPE, ESHAPE),
    ("cin_up with x2 NULL", _mut(cin_up=32), ESHAPE, ESHAPE),
    ("cin_up % 32", _mut(cin_up=16, x2="x2"), ESHAPE, ESHAPE),
    ("cin_up >= cin", _mut(cin_up=64, x2="x2"), ESHAPE, ESHAPE),
    ("cin_up, odd H", _mut(cin_up=32, x2="x2", H=5), ESHAPE, ESHAPE),
    ("cin_up, odd W", _mut(cin_up=32, x2="x2", W=7), ESHAPE, ESHAPE),
    ("F32 out_dtype BF16", _mut(out_dtype=BF16), EDTYPE, None),
    ("F32 with dec_out", _mut(dec_out="dec", dec_stride=32.0), EDTYPE, None),
    ("plane out_dtype neither F32 nor dtype", _mut(out_dtype="other"), None, EDTYPE),
    ("plane 3x3 with out_dtype F32", _mut(k=3, out_dtype=F32), None, ESHAPE),
    ("dec_out with cout % 3", _mut(dec_out="dec", dec_stride=32.0, out_dtype=F32), EDTYPE, ESHAPE),
    ("plane output cout % 8", _mut(cout=60), None, ESHAPE),
    ("unknown dtype", _mut(dtype=7, out_dtype=7), EDTYPE, EDTYPE),
]


@pytest.mark.parametrize("dtype", [F32, BF16, F32X3, F32H2], ids=["F32", "BF16", "F32X3", "F32H2"])
def test_conv_error_contract(dtype):
    """For every invalid descriptor: yv3_conv2d returns the documented YV3_E* code, yv3_conv2d_form and yv3_conv2d_launches return the
    same code (include/yv3.h) -- except for an unbound output, which the query does not require -- and the NaN-filled y is untouched."""
    lib = _lib()
    B, H, W, cin, cout = 1, 4, 4, 64, 64
    tdt = torch.float32 if dtype == F32 else engine._TORCH_DTYPE[dtype]
    big = 4 * 3 * B * H * W * 256                                   # generous: nothing here may be read or written at all
    bufs = {k: torch.zeros(big, dtype=tdt, device="cuda") for k in ("x", "x2", "w")}
    bufs["beta"] = torch.zeros(256, device="cuda")
    bufs["dec"] = torch.full((big,), NAN, device="cuda")
    y = torch.full((big,), NAN, dtype=tdt, device="cuda")
    ptrs = {k: v.data_ptr() for k, v in bufs.items()}
    ptrs["other"] = F32X3 if dtype == F32H2 else F32H2
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")

    def base():
        d = _ffi.ConvDesc()
        d.x, d.w, d.beta, d.y = ptrs["x"], ptrs["w"], ptrs["beta"], y.data_ptr()
        d.B, d.H, d.W, d.cin, d.cout, d.cout_pad, d.k, d.stride = B, H, W, cin, cout, cout, 1, 1
        d.act, d.dtype, d.out_dtype, d.flags = cr.ACT_LEAKY, dtype, dtype, flags.data_ptr()
        return d

    d = base()
    assert lib.yv3_conv2d_form(ctypes.byref(d)) == 0 and lib.yv3_conv2d_launches(ctypes.byref(d)) == 1
    failures = []
    for name, mutate, code_f32, code_planes in ERROR_CASES:
        want = code_f32 if dtype == F32 else code_planes
        if want is None:
            continue
        d = base()
        mutate(d, ptrs)
        got = (lib.yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), lib.yv3_conv2d_form(ctypes.byref(d)),
               lib.yv3_conv2d_launches(ctypes.byref(d)))
        if name.startswith("y NULL"):
            ok = got[0] == want and got[1] == 0 and got[2] == 1      # the query does not need a bound output
        else:
            ok = got == (want, want, want)
        if not ok:
            failures.append("%s: launch / form / launches = %s, expected %d" % (name, got, want))
    torch.cuda.synchronize()
    assert not failures, "\n".join(failures)
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(bufs["dec"]).all()) and int(flags.item()) == 0
