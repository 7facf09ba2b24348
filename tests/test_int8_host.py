"""Host side of the I8 math mode (no GPU): the definition's pieces in tests/int8_ref.py and their twins in yolo_v3_amd.engine, the
calibration bookkeeping, the mode checks, the library's entry points and selection, and the emulated network as a record."""
import copy
import ctypes
import ctypes.util
import os
import pickle
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import oracle_cpu as oc
from yolo_v3_amd import _ffi, arch, engine, synth, YoloNet, Yv3Error, I8
from tests import int8_ref as ir

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PTR = 0x7f0000000000          # a non-NULL pointer for descriptors that are only queried


# ----------------------------------------------------------------------------- weights
def test_weight_quantisation_properties_and_engine_twin():
    rng = np.random.default_rng(1)
    w = (rng.standard_normal((64, 128, 3, 3)) * 0.05).astype(F32)
    w[5] = 0.0                                                  # an all-zero filter
    w[6, :, :, :] *= 1e-6
    s_in = ir.input_scales(128, 0.031)
    qw, sw = ir.quantize_weights(w, s_in)
    eq, es = engine.quantize_weight_i8(w, s_in)
    assert np.array_equal(qw, eq) and np.array_equal(sw.view(np.int32), es.view(np.int32)), "engine.pack_conv's quantisation differs from the restatement"
    assert qw.dtype == F32 and np.array_equal(qw, np.rint(qw)) and np.abs(qw).max() == 127
    nz = [o for o in range(64) if o != 5]
    assert (np.abs(qw[nz]).reshape(len(nz), -1).max(axis=1) == 127).all(), "each non-zero filter reaches +-127"
    assert sw[5] == 1.0 and not qw[5].any()
    w1 = (w * s_in[None, :, None, None]).astype(np.float64)
    err = np.abs(sw.astype(np.float64)[:, None, None, None] * qw - w1)
    assert (err <= sw.astype(np.float64)[:, None, None, None] / 2 * (1 + 1e-6)).all(), "sw * qw is within sw / 2 of w'"


def test_concat_folding_equals_scaling_each_half():
    rng = np.random.default_rng(2)
    w = (rng.standard_normal((64, 384, 1, 1)) * 0.1).astype(F32)
    s_in = ir.input_scales(384, 0.02, cin_up=128, s_route=0.3)
    assert (s_in[:128] == F32(0.02)).all() and (s_in[128:] == F32(0.3)).all()
    qw, sw = ir.quantize_weights(w, s_in)
    halves = np.concatenate(((w[:, :128] * F32(0.02)).astype(F32), (w[:, 128:] * F32(0.3)).astype(F32)), axis=1)
    q2, s2 = ir.quantize_weights(halves, np.ones(384, dtype=F32))
    assert np.array_equal(qw, q2) and np.array_equal(sw, s2)
    specs = arch.conv_specs(80)
    g = arch.wiring(specs)
    sc = {n: 0.01 * (k + 1) for k, n in enumerate(engine.int8_scale_names(specs))}
    for i, up, route in ((60, "up1.conv", "feature.mlist.23.conv2"), (68, "up2.conv", "feature.mlist.14.conv2")):
        s = engine.int8_input_scales(specs, g, sc, i)
        cu = specs[i].cin - (512 if i == 60 else 256)
        assert s.shape == (specs[i].cin,) and (s[:cu] == F32(sc[up])).all() and (s[cu:] == F32(sc[route])).all()
    w_ = ir.wiring(specs)
    assert all(w_[i] == (g[i][0], g[i][1], g[i][3]) for i in range(1, 75)), "the restated wiring and the engine's graph differ"


# ----------------------------------------------------------------------------- arithmetic
def test_numpy_fmaf_equals_libm():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(3)
    n = 30000
    a = (rng.standard_normal(n) * rng.choice([1e-3, 1.0, 1e4, 1e8], n)).astype(F32)
    b = rng.standard_normal(n).astype(F32)
    c = rng.standard_normal(n).astype(F32)
    k = n // 3                                                        # cancelling: c = -round(a b), and its neighbours
    c[:k] = -(a[:k].astype(np.float64) * b[:k]).astype(F32)
    c[k // 2:k] = np.nextafter(c[k // 2:k], F32(np.inf))
    a[k:k + 1000] = rng.integers(-2 ** 27, 2 ** 27, 1000).astype(F32)  # integer sums times a small multiplier, as in the epilogue
    got = ir.fmaf(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=F32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "%d mismatches" % int((got.view(np.int32) != want.view(np.int32)).sum())
    plain = (a.astype(np.float64) * b + c).astype(F32)
    print("i8 host | fmaf: 0 of %d differ from libm (plain float64: %d)" % (n, int((plain.view(np.int32) != want.view(np.int32)).sum())))


def test_int_to_float_rounds_to_nearest_even():
    v = np.array([2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 24 + 2], dtype=np.int32).astype(F32)
    assert v.tolist() == [2.0 ** 24, 2.0 ** 24 + 4, -(2.0 ** 24), 2.0 ** 24 + 2]


def test_epilogue_clip_edges_and_ties():
    one = np.ones(1, dtype=F32)
    zero = np.zeros(1, dtype=F32)
    q = lambda acc, **kw: ir.epilogue(np.array([[acc]], dtype=np.int32), kw.pop("m", one), kw.pop("b", zero), kw.pop("s_out", 1.0), **kw)[0, 0]
    assert q(5, m=0.5 * one) == 2 and q(7, m=0.5 * one) == 4 and q(-5, m=5.0 * one) == -2           # ties to even (-25 * 0.1 = -2.5 -> -2)
    assert q(127) == 127 and q(128) == 127 and q(10 ** 9) == 127 and q(-(10 ** 9)) == -127 and q(-1271) == -127 and q(-1274) == -127
    assert q(-1264) == -126                                                                    # leaky: -126.4
    assert q(3, s_out=0.5) == 6 and q(100, s_out=0.5) == 127
    r = np.array([[-127]], dtype=np.int8)
    assert ir.epilogue(np.array([[100]], dtype=np.int32), one, zero, 1.0, r, 0.5)[0, 0] == 36      # 100 - 63.5 = 36.5 -> 36
    assert ir.epilogue(np.array([[0]], dtype=np.int32), one, zero, 1.0, r, 2.0)[0, 0] == -127      # the residual is added after the activation
    assert ir.quantize_act(np.array([0.5, 1.5, -0.5, -0.0, 1e9, -1e9, np.nan], dtype=F32), 1.0).tolist() == [0, 2, 0, 0, 127, -127, 0]


def test_layer_at_pixels_equals_conv_layer():
    """int8_ref.layer_at_pixels on gathered windows == int8_ref.conv_layer at those pixels, for every output pixel of three small layers:
    3x3 with a residual (halos on all edges), 3x3 stride 2 on a non-square picture with odd output sizes, and the two-source 1x1."""
    rng = np.random.default_rng(5)
    for cin, cout, k, stride, B, H, W, res, cin_up in ((64, 64, 3, 1, 2, 5, 7, True, 0), (64, 128, 3, 2, 2, 10, 6, False, 0), (192, 64, 1, 1, 2, 6, 10, False, 64)):
        x = rng.integers(-127, 128, size=(B, H // 2 if cin_up else H, W // 2 if cin_up else W, cin_up or cin)).astype(np.int8)
        x2 = rng.integers(-127, 128, size=(B, H, W, cin - cin_up)).astype(np.int8) if cin_up else None
        w = (rng.standard_normal((cout, cin, k, k)) * 0.05).astype(F32)
        s_in = ir.input_scales(cin, 0.02, cin_up, 0.05 if cin_up else None)
        alpha, beta = rng.uniform(0.5, 1.5, cout).astype(F32), rng.uniform(-1.0, 1.0, cout).astype(F32)
        s_out = 0.0017 * np.sqrt(k * k * cin)                           # ~3 sigma of the activation at 127
        pad = (k - 1) // 2
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        r = rng.integers(-127, 128, size=(B, Ho, Wo, cout)).astype(np.int8) if res else None
        want = ir.conv_layer(x, w, s_in, alpha, beta, s_out, stride, x2, r, 0.03 if res else None)
        assert want.shape == (B, Ho, Wo, cout) and len(np.unique(want)) > 50
        pix = np.stack(np.meshgrid(np.arange(B), np.arange(Ho), np.arange(Wo), indexing="ij"), axis=-1).reshape(-1, 3)
        pix = pix[rng.permutation(len(pix))]                             # any order, every pixel
        patches = ir.gather_patches(x, pix, k, stride, x2)
        assert patches.shape == (len(pix), k, k, cin) and patches.dtype == np.int8
        got = ir.layer_at_pixels(patches, w, s_in, alpha, beta, s_out, r[pix[:, 0], pix[:, 1], pix[:, 2]] if res else None, 0.03 if res else None)
        assert np.array_equal(got, want[pix[:, 0], pix[:, 1], pix[:, 2]].astype(F32)), (cin, cout, k, stride)
        if k == 3:                                                       # the corner windows are zero outside the picture, and only there
            b, yi, xi, inside = ir.patch_index(np.array([[0, 0, 0], [B - 1, Ho - 1, Wo - 1]]), k, stride, H, W)
            assert not inside[0, 0].any() and not inside[0, :, 0].any() and inside[0, 1:, 1:].all()
            assert inside[1].sum() == (4 if stride == 1 else 9)            # (stride 2 on an even picture: the last window ends at the last row)


# ----------------------------------------------------------------------------- calibration and the mode's checks
def _names():
    return engine.int8_scale_names(arch.conv_specs(3))


def test_calibration_bookkeeping_with_a_stubbed_engine(monkeypatch):
    net = YoloNet((64, 64), numClass=3)
    names = _names()
    assert len(names) == 69 and len(set(names)) == 69 and names == ir.scale_names(arch.conv_specs(3))
    assert net.int8_scales is None
    batches = [{n: torch.full((1, 2, 2, 4), -float(k + 1)) for k, n in enumerate(names)},
               {n: torch.full((1, 2, 2, 4), 254.0 if k == 7 else 0.5) for k, n in enumerate(names)}]
    batches[0][names[9]] = torch.zeros(1, 2, 2, 4)
    batches[1][names[9]] = torch.zeros(1, 2, 2, 4)
    it = iter(batches)
    monkeypatch.setattr(YoloNet, "_int8_calibration_outputs", lambda self, x: next(it))
    out = net.calibrate_int8([None, None])
    assert out is net.int8_scales and sorted(out) == sorted(names)
    for k, n in enumerate(names):
        want = 1.0 if k == 9 else float(F32(254.0 if k == 7 else k + 1) / F32(127.0))        # the running max over both batches; 1 for a dead tensor
        assert out[n] == want, (n, out[n], want)
    with pytest.raises(Yv3Error):
        net.calibrate_int8([])
    # a plain attribute: travels with pickle and deepcopy, is no state_dict key; changing it changes the packing signature
    assert pickle.loads(pickle.dumps(net)).int8_scales == out and copy.deepcopy(net).int8_scales == out
    assert not any("int8" in k for k in net.state_dict())
    net.load_state_dict(YoloNet((64, 64), numClass=3).state_dict(), strict=True)
    assert net.int8_scales == out
    eng = engine.Engine(net, I8)
    s1 = eng._signature()
    assert eng._signature() == s1
    net.int8_scales = dict(out, **{names[20]: out[names[20]] * 2})
    assert eng._signature() != s1, "changed scales must signal a re-pack"
    assert engine.Engine(net, _ffi.BF16)._signature() == engine.Engine(net, _ffi.BF16)._signature()


def test_i8_without_scales_raises_and_says_calibrate():
    net = YoloNet((64, 64), numClass=3)
    with pytest.raises(Yv3Error, match="calibrate_int8"):
        net.math_mode = I8
    assert net.math_mode != I8
    net.int8_scales = {n: 0.1 for n in _names()[:-1]}              # incomplete
    with pytest.raises(Yv3Error, match="calibrate_int8"):
        net.math_mode = I8
    net.int8_scales = {n: 0.1 for n in _names()}
    net.int8_scales[_names()[3]] = 0.0                             # not positive
    with pytest.raises(Yv3Error):
        net.math_mode = I8
    net.int8_scales[_names()[3]] = 0.1
    net.math_mode = I8
    assert net.math_mode == I8
    net.int8_scales = None                                         # taken away again: the engine's signature refuses
    with pytest.raises(Yv3Error, match="calibrate_int8"):
        engine.Engine(net, I8)._signature()


def test_i8_is_rejected_for_training_and_for_the_frozen_prefix():
    from yolo_v3_amd import backprop
    net = YoloNet((96, 96), numClass=3)
    net.backprop_math = I8
    with pytest.raises(Yv3Error) as e:
        backprop.backprop_math(net)
    assert e.value.code == _ffi.EINVAL
    net.backprop = True
    with pytest.raises(Yv3Error) as e:                    # the training entry point itself: CPU tensors, nothing packed, nothing launched
        net(torch.zeros(1, 3, 96, 96), torch.zeros(1, 1, 5))
    assert e.value.code == _ffi.EINVAL
    assert I8 not in backprop.PREFIX_MODE and I8 not in backprop.PREFIX_MODE.values()
    with pytest.raises(Yv3Error, match="prefix"):
        net.prefix_engine(I8, 10)
    with pytest.raises(Yv3Error):
        engine.to_planes(torch.zeros(1, 2, 2, 64), I8)


# ----------------------------------------------------------------------------- the library
def test_mode_code_header_exports_and_descriptor():
    with open(os.path.join(REPO, "include", "yv3.h")) as f:
        m = re.search(r"^#define\s+YV3_I8\s+(\d+)", f.read(), re.M)
    import yolo_v3_amd
    assert m and int(m.group(1)) == yolo_v3_amd.I8 == _ffi.I8 == 6
    assert engine.PLANES[I8] == 1 and engine._TORCH_DTYPE[I8] == torch.int8
    lib = _ffi.lib()
    assert "yv3_quantize_bf16_i8" in _ffi.EXPORTS and lib.yv3_quantize_bf16_i8 is not None
    fields = dict(_ffi.ConvDesc._fields_)
    assert fields["s_res"] is ctypes.c_float and fields["inv_s_out"] is ctypes.c_float
    assert lib.yv3_pack_conv_weight(PTR, None, 64, 64, 3, 64, I8, None) == _ffi.EINVAL
    assert lib.yv3_pack_conv_weight(PTR, PTR, 64, 64, 4, 64, I8, None) == _ffi.ESHAPE
    assert lib.yv3_pack_conv_weight(PTR, PTR, 64, 32, 1, 64, I8, None) == _ffi.ESHAPE           # cin must be a multiple of 64
    assert lib.yv3_quantize_bf16_i8(None, PTR, 8, 1.0, None) == _ffi.EINVAL and lib.yv3_quantize_bf16_i8(PTR, PTR, 0, 1.0, None) == 0


def _desc(dtype, cin, cout, k=1, stride=1, B=8, H=52, W=52, cin_up=0, out_dtype=None):
    d = _ffi.ConvDesc()
    d.x, d.w, d.beta, d.alpha, d.y = PTR, PTR + 0x100, PTR + 0x200, PTR + 0x300, PTR + 0x400
    d.x2 = PTR + 0x500 if cin_up else None
    d.B, d.H, d.W, d.cin, d.cin_up, d.cout, d.cout_pad, d.k, d.stride = B, H, W, cin, cin_up, cout, cout, k, stride
    d.act, d.dtype, d.out_dtype = _ffi.ACT_LEAKY, dtype, dtype if out_dtype is None else out_dtype
    return d


def test_i8_selection_is_the_bf16_choice_for_the_layers_bytes():
    """Through conv_select.cpp (nothing launched): an int8 layer of C input channels takes the tile of the bf16 layer of C / 2, for every
    int8 layer shape of the network at three batch sizes; shapes and formats the int8 kernels do not take are refused."""
    lib = _ffi.lib()
    specs = arch.conv_specs(80)
    hw = arch.conv_output_hw(416)
    g = arch.wiring(specs)
    n = 0
    for B in (1, 16, 64):
        for i in engine.int8_layers(specs):
            sp, (ho, wo) = specs[i], hw[i]
            h, w = ho * sp.stride, wo * sp.stride
            cu = g[i][2]
            a = _ffi.conv2d_kernel(_desc(I8, sp.cin, sp.cout, sp.k, sp.stride, B, h, w, cu))
            b = _ffi.conv2d_kernel(_desc(_ffi.BF16, sp.cin // 2, sp.cout, sp.k, sp.stride, B, h, w, cu // 2))
            assert a == b, (sp.name, B, a, b)
            assert lib.yv3_conv2d_form(ctypes.byref(_desc(I8, sp.cin, sp.cout, sp.k, sp.stride, B, h, w, cu))) == 0
            n += 1
    assert n == 3 * 68
    q = lambda d: lib.yv3_conv2d_launches(ctypes.byref(d))
    assert q(_desc(I8, 64, 64)) == 1 and q(_desc(I8, 64, 64, out_dtype=_ffi.BF16)) == 1
    assert q(_desc(I8, 32, 64)) == _ffi.ESHAPE and q(_desc(I8, 96, 64)) == _ffi.ESHAPE and q(_desc(I8, 192, 64, cin_up=32)) == _ffi.ESHAPE
    assert q(_desc(I8, 64, 64, out_dtype=_ffi.F32)) == -4 and q(_desc(I8, 64, 64, out_dtype=_ffi.F16)) == -4
    assert q(_desc(_ffi.BF16, 64, 64, out_dtype=I8)) == -4


# ----------------------------------------------------------------------------- the emulated network: a record, not a bar
def test_emulated_network_runs_and_reports_its_logit_error():
    """SW-1 weights, 64 x 64, one image: the CPU oracle's fp32 arithmetic for the seven convolutions that are not int8, int8_ref for the
    68 that are, scales from the oracle's own activations on this image.  Finite logits; the error against the fp32 oracle is printed
    (recorded in DESIGN.md 8g)."""
    specs = arch.conv_specs(80)
    sd, _ = oc.state_dict_from_stream(synth.weight_stream(80), 80)
    x = torch.from_numpy(synth.images(1, 64, 4242))
    taps = []
    with torch.no_grad():
        want = oc.head_logits(sd, x, taps)
    tap = {n: t.permute(0, 2, 3, 1).contiguous().numpy() for n, t in taps}
    names = ir.scale_names(specs)
    scales = {n: float(F32(np.abs(tap[n]).max()) / F32(127.0)) for n in names}
    params = {}
    for i in ir.int8_layers(specs):
        p = specs[i].name
        a, b = ir.fold_bn(sd[p + ".bn.weight"].numpy(), sd[p + ".bn.bias"].numpy(), sd[p + ".bn.running_mean"].numpy(), sd[p + ".bn.running_var"].numpy())
        params[i] = (sd[p + ".conv.weight"].numpy(), a, b)
    out = ir.run_layers(specs, params, scales, ir.quantize_act(tap[names[0]], scales[names[0]]))
    worst, clipped = 0.0, []
    for i, ref in zip([i for i, sp in enumerate(specs) if not sp.bn], want):
        xin = torch.from_numpy(out[i - 1].astype(F32) * F32(scales[specs[i - 1].name])).permute(0, 3, 1, 2)
        with torch.no_grad():
            lg = F.conv2d(xin, sd[specs[i].name + ".weight"], sd[specs[i].name + ".bias"])
        assert bool(torch.isfinite(lg).all())
        e = float((lg - ref).abs().max() / ref.abs().max())
        rms = float((lg - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
        print("i8 host | emulated network | %s: max |d| / max |ref| = %.4f, rms(d) / rms(ref) = %.4f" % (specs[i].name, e, rms))
        worst = max(worst, e)
    sat = np.mean([float((np.abs(out[i]) == 127).mean()) for i in ir.int8_layers(specs)])
    print("i8 host | emulated network | worst head max |d| / max |ref| = %.4f | mean share of values at +-127: %.5f" % (worst, sat))
