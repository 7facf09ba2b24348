"""The I8 math mode's kernels through the C-ABI, bit for bit against the definition (tests/int8_ref.py): the int8
implicit-GEMM convolution on v_mfma_i32_32x32x32_i8 -- random int8 inputs and weights over the full range, +-127 included, at the
smallest shapes at which each path can still go wrong, on the tile the selector picks and on every forced one-plane tile -- its
bf16-output form, and the bf16 -> int8 quantise kernel; then every tile again on grids of 11 to 48 workgroups (GRID_CASES: three or more
row tiles, up to eight channel tiles, a remapped workgroup index), each forced launch held to the tile it asked for.  Integer sums are exact, so a wrong lane map, halo, stride or K order cannot
hide inside a tolerance."""
import ctypes
import time

import numpy as np
import pytest
import torch

from yolo_v3_amd import _ffi
from tests import int8_ref as ir

pytestmark = pytest.mark.gpu

I8, BF16 = _ffi.I8, _ffi.BF16
CANARY = 4096
UNWRITTEN = -128                      # never produced by the kernels: what the output buffer is filled with
SENTINEL = 85                         # the bytes behind it
CODES = (1, 2, 3, 5, 6, 7, 8, 9, 11, 13, 14, 15, 16)       # forced tile codes of the one-plane kernels (a declined code gives the default's tile)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "needs the MI355X"
    torch.cuda.set_device(0)
    yield
    torch.cuda.synchronize()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Layer:
    """One int8 convolution: integer operands over the full range, an epilogue whose results spread over [-127, 127] and beyond."""

    def __init__(self, cin, cout, k=1, stride=1, B=1, H=13, W=13, res=False, cin_up=0, seed=0, extreme=False):
        rng = np.random.default_rng(seed)
        self.cin, self.cout, self.k, self.stride, self.B, self.H, self.W, self.cin_up = cin, cout, k, stride, B, H, W, cin_up
        pad = (k - 1) // 2
        self.Ho, self.Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        K = k * k * cin
        if extreme:
            # every operand at +-127: x = +127, each filter -127 at ~3 % of its positions -- interior sums of 16129 * (K - 2 n) ~ 1.4e8 > 2^24 are
            # not representable in fp32 (one ulp = 16); b cancels each channel's rounded interior sum, so that one ulp of (float)acc moves q by 1
            x = np.full((B, H, W, cin), 127, dtype=np.int8)
            qw = np.where(rng.random((cout, cin, k, k)) < 0.03, -127.0, 127.0).astype(np.float32)
            interior = 127 * qw.reshape(cout, -1).astype(np.int64).sum(axis=1)
            assert (np.abs(interior) > 2 ** 24).all() and (interior % 16 != 0).any()
            self.m = np.ones(cout, dtype=np.float32)
            self.b = (-(interior.astype(np.int32).astype(np.float32)) + 16.0 * (np.arange(cout) % 41 - 20)).astype(np.float32)
            self.s_out = 16.0
        else:
            x = rng.integers(-127, 128, size=(B, H // 2 if cin_up else H, W // 2 if cin_up else W, cin_up or cin), dtype=np.int64).astype(np.int8)
            qw = rng.integers(-127, 128, size=(cout, cin, k, k)).astype(np.float32)
            x.reshape(-1)[:64] = 127; x.reshape(-1)[64:128] = -127
            qw.reshape(-1)[:64] = 127.0; qw.reshape(-1)[64:128] = -127.0
            self.s_out = 0.37
            self.m = (rng.uniform(0.5, 1.5, cout) * 60.0 * self.s_out / (np.sqrt(K) * 5376.0)).astype(np.float32)
            self.b = (rng.uniform(-8.0, 8.0, cout) * self.s_out).astype(np.float32)
        self.x, self.qw = x, qw
        self.x2 = rng.integers(-127, 128, size=(B, H, W, cin - cin_up)).astype(np.int8) if cin_up else None
        self.res = rng.integers(-127, 128, size=(B, self.Ho, self.Wo, cout)).astype(np.int8) if res else None
        self.s_res = 0.21 if res else 0.0
        self.inv_s_out = float(np.float32(1.0) / np.float32(self.s_out))
        # device side
        self.d_x, self.d_x2, self.d_res = _dev(x), (_dev(self.x2) if cin_up else None), (_dev(self.res) if res else None)
        self.d_m, self.d_b = _dev(self.m), _dev(self.b)
        wq = _dev(qw)
        self.wp = torch.full((cout * K + CANARY,), SENTINEL, dtype=torch.int8, device="cuda")
        _ffi.check(_ffi.lib().yv3_pack_conv_weight(wq.data_ptr(), self.wp.data_ptr(), cout, cin, k, cout, I8, _ffi.stream_ptr()), "yv3_pack_conv_weight")
        torch.cuda.synchronize()
        assert bool((self.wp[cout * K:] == SENTINEL).all()), "the weight pack wrote past its image"
        assert torch.equal(torch.sort(self.wp[:cout * K].view(-1))[0].cpu(), torch.sort(torch.from_numpy(qw.astype(np.int8)).view(-1))[0]), \
            "the packed image is not a permutation of the weights"

    def ref(self):
        acc = ir.conv_acc(ir.gather_input(self.x, self.x2), self.qw, self.stride)
        return acc, ir.epilogue(acc, self.m, self.b, self.s_out, self.res, self.s_res if self.res is not None else None)

    def desc(self, y, out_dtype=I8, code=0, big_tile_min=0):
        d = _ffi.ConvDesc()
        d.x, d.x2, d.w = self.d_x.data_ptr(), (self.d_x2.data_ptr() if self.d_x2 is not None else None), self.wp.data_ptr()
        d.alpha, d.beta = self.d_m.data_ptr(), self.d_b.data_ptr()
        d.residual, d.y = (self.d_res.data_ptr() if self.d_res is not None else None), (y.data_ptr() if y is not None else None)
        d.B, d.H, d.W, d.cin, d.cin_up = self.B, self.H, self.W, self.cin, self.cin_up
        d.cout, d.cout_pad, d.k, d.stride, d.act = self.cout, self.cout, self.k, self.stride, _ffi.ACT_LEAKY
        d.dtype, d.out_dtype = I8, out_dtype
        d.options = (code & 0xff) << _ffi.OPT_TILE_SHIFT
        d.big_tile_min = big_tile_min
        d.s_res, d.inv_s_out = self.s_res, self.inv_s_out
        return d

    def launch(self, out_dtype=I8, code=0, what="", big_tile_min=0):
        n = self.B * self.Ho * self.Wo * self.cout
        if out_dtype == I8:
            y = torch.full((n + CANARY,), UNWRITTEN, dtype=torch.int8, device="cuda")
            y[n:] = SENTINEL
        else:
            y = torch.full((n + CANARY,), float("nan"), dtype=torch.bfloat16, device="cuda")
        d = self.desc(y, out_dtype, code, big_tile_min)
        _ffi.check(_ffi.lib().yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()), "yv3_conv2d " + what)
        torch.cuda.synchronize()
        if out_dtype == I8:
            assert bool((y[n:] == SENTINEL).all()), "%s: wrote past the end of y" % what
            assert int((y[:n] == UNWRITTEN).sum()) == 0, "%s: %d output bytes not written (or -128 produced)" % (what, int((y[:n] == UNWRITTEN).sum()))
            return y[:n].cpu().numpy().reshape(self.B, self.Ho, self.Wo, self.cout).astype(np.float32)
        assert bool(torch.isnan(y[n:]).all()), "%s: wrote past the end of y" % what
        assert not bool(torch.isnan(y[:n]).any()), "%s: output elements not written" % what
        return y[:n].float().cpu().numpy().reshape(self.B, self.Ho, self.Wo, self.cout)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d of %d outputs differ, first at (b, y, x, c) = %s: got %s, want %s" % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


# name, constructor arguments.  The first six are the issue's shapes; the two "wide" ones give the 256-channel tiles something to run on.
CASES = [
    ("1x1_64to64_ragged", dict(cin=64, cout=64, B=1, H=13, W=13)),                                   # M = 169: a ragged last tile
    ("1x1_128to64_two_tiles", dict(cin=128, cout=64, B=2, H=13, W=13)),                              # M = 338 crosses a 256-row tile
    ("3x3_s1_64to128_res", dict(cin=64, cout=128, k=3, B=2, H=13, W=13, res=True)),                  # halos on all four edges, image boundaries inside a tile
    ("3x3_s2_64to128_nonsquare", dict(cin=64, cout=128, k=3, stride=2, B=1, H=20, W=28)),            # -> 10 x 14: swapped H / W would show
    ("1x1_upcat_64+128to128", dict(cin=192, cout=128, cin_up=64, B=1, H=10, W=14)),                  # x 5x7x64 upsampled, x2 10x14x128: three chunks
    ("3x3_1024to64_all_127", dict(cin=1024, cout=64, k=3, B=1, H=4, W=4, extreme=True)),             # |acc| > 2^24, the longest K loop
    ("3x3_s1_64to256_res_wide", dict(cin=64, cout=256, k=3, B=2, H=13, W=13, res=True)),
    ("1x1_upcat_128+128to256_wide", dict(cin=256, cout=256, cin_up=128, B=2, H=10, W=14)),
]


@pytest.mark.parametrize("name,kw", CASES, ids=[c[0] for c in CASES])
def test_int8_conv_bitwise(name, kw):
    """yv3_conv2d in YV3_I8 == the definition, on the selector's tile and on every forced tile code, int8 and bf16 output alike."""
    layer = Layer(seed=len(name) * 13 + 1, **kw)
    acc, want = layer.ref()
    print("i8 conv | %s | %s | max |acc| %d | outputs at +-127: %.1f %% | distinct q: %d" % (
        name, _ffi.conv2d_kernel(layer.desc(None)), int(np.abs(acc.astype(np.int64)).max()), 100.0 * float((np.abs(want) == 127).mean()), len(np.unique(want))))
    assert len(np.unique(want)) > 20, "the reference output does not spread: the case checks nothing"
    _same(layer.launch(what=name), want, name + " default")
    _same(layer.launch(BF16, what=name + " bf16 out"), want, name + " bf16 out")
    seen = set()
    for code in CODES:
        d = layer.desc(None, code=code)
        line = _ffi.conv2d_kernel(d)
        if line in seen:
            continue
        seen.add(line)
        _same(layer.launch(code=code, what="%s code %d" % (name, code)), want, "%s code %d (%s)" % (name, code, line))
    line = _ffi.conv2d_kernel(layer.desc(None, big_tile_min=1))             # the eight-wave ping-pong tile on its 6-deep ring: no code forces it, a threshold of one tile does
    if layer.cout % 128 == 0:
        assert line.startswith("256x128_W8_PP6") and line not in seen, line
        seen.add(line)
        _same(layer.launch(big_tile_min=1, what=name + " big_tile_min 1"), want, "%s big_tile_min 1 (%s)" % (name, line))
    print("i8 conv | %s | forced tiles run: %s" % (name, sorted(seen)))


# Many tiles in both directions: three or more row tiles of every tile height (the last one ragged), two to eight channel tiles, 12 to 48
# workgroups -- yv3_xcd_remap permutes the workgroup index from 8 workgroups on, and with a count that is no multiple of 8 both of its
# branches run.  On these shapes the selector accepts every code of CODES and big_tile_min = 1 (256 CUs, checked on the host): the test
# asserts the tile it asked for, so a declined code cannot pass on the default's tile.
TILE_OF_CODE = {1: "256x128_W8", 2: "128x128_W8", 3: "128x128_W4", 5: "256x128_W4", 6: "256x256", 7: "256x128_W4_ROLL", 8: "256x256_ROLL",
                9: "256x256_ROLL4", 11: "192x256_ROLL", 13: "256x256_PP3", 14: "256x256_PP4", 15: "192x256_PP3", 16: "192x256_PP4"}
BF16_OUT_CODES = (14, 16)
GRID_CASES = [
    ("3x3_128to1024_res_grid", dict(cin=128, cout=1024, k=3, B=4, H=13, W=13, res=True), CODES),      # M = 676: 3 x 256 / 4 x 192 / 6 x 128 rows, 4 or 8 channel tiles
    ("1x1_1024to512_grid", dict(cin=1024, cout=512, B=4, H=13, W=13), CODES),                         # 16 chunks of 64 on the 3-, 4- and 6-deep rings
    ("1x1_256to512_grid", dict(cin=256, cout=512, B=5, H=13, W=13), CODES),                           # M = 845: four row tiles of 256; 4 chunks < the 6-deep ring
    ("3x3_s2_64to256_grid", dict(cin=64, cout=256, k=3, stride=2, B=3, H=38, W=26), CODES),           # -> 19 x 13 (M = 741): stride 2, non-square, odd output sizes
    ("1x1_upcat_128+256to256_grid", dict(cin=384, cout=256, cin_up=128, B=5, H=14, W=10), CODES),     # M = 700: the two-source gather across row tiles and images
    ("3x3_512to1024_res_timed", dict(cin=512, cout=1024, k=3, B=4, H=13, W=13, res=True), BF16_OUT_CODES),   # K = 4608: DESIGN.md 8g's 1821 TOP/s layer
    ("1x1_128to64_grid", dict(cin=128, cout=64, B=8, H=13, W=13), ()),                                # M = 1352: 11 workgroups of the one 64-channel tile (128x64)
]


def _tile(line):
    return line.split()[0]


@pytest.mark.parametrize("name,kw,codes", GRID_CASES, ids=[c[0] for c in GRID_CASES])
def test_int8_conv_grid_bitwise(name, kw, codes):
    """Every int8 tile on a grid of 12 to 48 workgroups, whole tensor against the definition: the selector's tile, every forced code and
    big_tile_min = 1 with int8 output; the selector's tile and codes 14 and 16 (the ping-pong tiles of the timed plans) with bf16 output.
    Each forced launch must run the tile it was asked for."""
    t0 = time.time()
    layer = Layer(seed=len(name) * 13 + 1, **kw)
    acc, want = layer.ref()
    t_ref = time.time() - t0
    default = _ffi.conv2d_kernel(layer.desc(None))
    print("i8 grid | %s | M = %d | %s | max |acc| %d | outputs at +-127: %.1f %% | distinct q: %d" % (
        name, layer.B * layer.Ho * layer.Wo, default, int(np.abs(acc.astype(np.int64)).max()), 100.0 * float((np.abs(want) == 127).mean()), len(np.unique(want))))
    assert len(np.unique(want)) > 20, "the reference output does not spread: the case checks nothing"
    assert _ffi.conv2d_kernel(layer.desc(None, out_dtype=BF16)) == default
    _same(layer.launch(what=name), want, name + " default (%s)" % default)
    _same(layer.launch(BF16, what=name + " bf16 out"), want, name + " bf16 out (%s)" % default)
    ran = [default]
    for code in codes:
        line = _ffi.conv2d_kernel(layer.desc(None, code=code))
        assert _tile(line) == TILE_OF_CODE[code], "%s: code %d was declined: the selector gives %s" % (name, code, line)
        ran.append(line)
        _same(layer.launch(code=code, what="%s code %d" % (name, code)), want, "%s code %d (%s)" % (name, code, line))
        if code in BF16_OUT_CODES:
            assert _ffi.conv2d_kernel(layer.desc(None, out_dtype=BF16, code=code)) == line
            _same(layer.launch(BF16, code=code, what="%s code %d bf16 out" % (name, code)), want, "%s code %d bf16 out (%s)" % (name, code, line))
    if layer.cout % 128:
        assert _tile(default) == "128x64" and not codes, default          # 64 output channels: the one tile there is
    else:
        line = _ffi.conv2d_kernel(layer.desc(None, big_tile_min=1))
        assert _tile(line) == "256x128_W8_PP6", "%s: big_tile_min = 1 was declined: the selector gives %s" % (name, line)
        ran.append(line)
        _same(layer.launch(big_tile_min=1, what=name + " big_tile_min 1"), want, "%s big_tile_min 1 (%s)" % (name, line))
        assert len(set(ran[1:])) == len(codes) + 1, ran
    print("i8 grid | %s | %d launches, %.2f s (numpy reference %.2f s) | lines run: %s" % (
        name, len(ran) + 1 + sum(c in BF16_OUT_CODES for c in codes), time.time() - t0, t_ref, "; ".join(ran)))


def test_int8_conv_extreme_case_exercises_int_to_float_rounding():
    """The all-+-127 case is sensitive to how (float)acc rounds: with truncation instead of round-to-nearest-even the reference itself moves."""
    layer = Layer(seed=79, **dict(CASES)["3x3_1024to64_all_127"])
    acc, want = layer.ref()
    trunc = (np.sign(acc) * (np.abs(acc.astype(np.int64)) // 16 * 16)).astype(np.float64).astype(np.float32)
    t = ir.fmaf(trunc, layer.m, layer.b)
    v = np.maximum(t, (np.float32(0.1) * t).astype(np.float32))
    other = np.clip(np.rint((v * np.float32(layer.inv_s_out)).astype(np.float32)), -127, 127)
    assert int((other != want).sum()) > 0
    _same(layer.launch(what="extreme"), want, "extreme")


def test_int8_desc_errors():
    """Shapes and formats the int8 kernels do not take are refused before anything is launched."""
    layer = Layer(seed=3, cin=64, cout=64, B=1, H=4, W=4)
    y = torch.zeros(4 * 4 * 64 * 4, dtype=torch.int8, device="cuda")
    lib = _ffi.lib()
    d = layer.desc(y); d.cin = 32
    assert lib.yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()) == _ffi.ESHAPE
    d = layer.desc(y, out_dtype=_ffi.F32)
    assert lib.yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()) == -4          # YV3_EDTYPE: the heads are BF16 launches
    d = layer.desc(y); d.options = _ffi.OPT_K3S1 | _ffi.OPT_WINO_ALWAYS
    assert lib.yv3_conv2d(ctypes.byref(d), _ffi.stream_ptr()) == 0           # (options of other modes' kernels are ignored)
    torch.cuda.synchronize()


def test_quantize_bf16_to_int8():
    """yv3_quantize_bf16_i8 at 2 x 6 x 10 x 64: ties (to even), values beyond +-127 s, negative zero, infinities, NaN -> 0."""
    rng = np.random.default_rng(11)
    n = 2 * 6 * 10 * 64
    for s in (0.25, 0.0371):
        x = torch.from_numpy((rng.standard_normal(n) * 40.0 * s).astype(np.float32)).bfloat16()
        ties = torch.tensor([(2 * k + 1) / 8.0 for k in range(-127, 127)]).bfloat16()                 # s = 0.25: x / s = k + 0.5 exactly, |.| <= 126.5
        x[:ties.numel()] = ties
        special = torch.tensor([0.0, -0.0, 127 * s, -127 * s, 127.4 * s, 127.6 * s, -128 * s, 1e4, -1e4, float("inf"), float("-inf"), float("nan"), 1e-30, -1e-30])
        x[300:300 + special.numel()] = special.bfloat16()
        xf = x.float().numpy()
        inv = float(np.float32(1.0) / np.float32(s))
        out = torch.full((n + CANARY,), UNWRITTEN, dtype=torch.int8, device="cuda")
        out[n:] = SENTINEL
        xd = x.cuda()
        _ffi.check(_ffi.lib().yv3_quantize_bf16_i8(xd.data_ptr(), out.data_ptr(), n, inv, _ffi.stream_ptr()), "yv3_quantize_bf16_i8")
        torch.cuda.synchronize()
        assert bool((out[n:] == SENTINEL).all())
        got, want = out[:n].cpu().numpy(), ir.quantize_act(xf, s)
        assert want.min() == -127 and want.max() == 127 and got.min() >= -127
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "s = %g: %d differ, first x = %r: got %d want %d" % (s, bad.size, xf[bad[0]], got[bad[0]], want[bad[0]])
        if s == 0.25:
            assert (want[:ties.numel()] % 2 == 0).all() and ties.numel() == 254, "ties must round to even"
    lib = _ffi.lib()
    assert lib.yv3_quantize_bf16_i8(None, out.data_ptr(), n, 1.0, None) == _ffi.EINVAL
    assert lib.yv3_quantize_bf16_i8(xd.data_ptr(), out.data_ptr(), n + 4, 1.0, None) == _ffi.ESHAPE
    assert lib.yv3_quantize_bf16_i8(xd.data_ptr(), out.data_ptr(), n, 0.0, None) == _ffi.EINVAL
