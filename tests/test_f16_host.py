"""The F16 math mode without a GPU: the bar its kernels are held to (tests/conv_ref_f16.py) -- pinned as the BF16 bar is in
tests/test_conv_ref_host.py: a correct fp32-accumulated stand-in passes it, wrong epilogues fail it --, the selection of an F16
descriptor (the BF16 descriptor's, query for query), the mode code, and the CPU evaluation of the mode's definition (tests/f16_ref.py)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from oracle import oracle_cpu as oc
from yolo_v3_amd import _ffi, synth
from tests import conv_ref as cr, conv_ref_f16 as cf, conv_select_grid as grid, f16_ref, helpers
from tests.test_conv_ref_host import BF16_SHAPES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f16(t):
    return t.half().float()


# ----------------------------------------------------------------------------- the rounding helper
def test_round_f16_f64_is_one_rounding():
    """Equal to torch's fp32 -> fp16 on 200 000 fp32 values over 10 decades down into the subnormals, ties to even, NOT double-rounded
    from float64, quantum 2^-24 below 2^-14, saturation at +-65504."""
    g = torch.Generator().manual_seed(1)
    v = (torch.rand(200000, generator=g) * 2 - 1) * 10.0 ** (torch.rand(200000, generator=g) * 10 - 9)        # 1e-9 .. 10
    assert int((v.abs() < 2.0 ** -14).sum()) > 50000 and int((v.abs() > 1e-2).sum()) > 30000
    assert torch.equal(cf.round_f16_f64(v.double()), _f16(v).double())
    ties = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(2.0 + 2.0 ** -10), 0.0, 2.0 ** -25, 3 * 2.0 ** -25], dtype=torch.float64)
    assert cf.round_f16_f64(ties).tolist() == [1.0, 1.0 + 2.0 ** -9, -2.0, 0.0, 0.0, 2.0 ** -23]
    assert torch.equal(cf.round_f16_f64(ties), _f16(ties.float()).double())
    just_over = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -40], dtype=torch.float64)          # fp32 first would land on the tie, then on 1.0
    assert cf.round_f16_f64(just_over).item() == 1.0 + 2.0 ** -10 and _f16(just_over.float()).item() == 1.0
    sub = torch.tensor([2.0 ** -24, 5 * 2.0 ** -24 + 2.0 ** -30, -(2.0 ** -14 - 2.0 ** -25 + 2.0 ** -40)], dtype=torch.float64)
    assert cf.round_f16_f64(sub).tolist() == [2.0 ** -24, 5 * 2.0 ** -24, -(2.0 ** -14)]
    big = torch.tensor([65504.0, 65519.0, 65520.0, 7e4, -1e30, float("inf")], dtype=torch.float64)
    assert cf.round_f16_f64(big).tolist() == [65504.0, 65504.0, 65504.0, 65504.0, -65504.0, 65504.0]


# ----------------------------------------------------------------------------- the bar: a correct stand-in passes, wrong epilogues fail
def _operands(cin, cout, k, s, B, H, W, res, alpha_none, seed):
    """tests/test_conv_ref_host._bf16_operands with fp16 operands: x, w, residual rounded to fp16; alpha (fan-in scale), beta fp32."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, lo, hi: torch.rand(shape, generator=g) * (hi - lo) + lo
    x = _f16(u((B, H, W, cin), -1.0, 1.0))
    w = _f16(u((cout, cin, k, k), -1.0, 1.0))
    alpha = None if alpha_none else u((cout,), 0.5, 1.5) / (cin * k * k) ** 0.5
    beta = u((cout,), -0.2, 0.2)
    Ho, Wo = cr.out_hw(H, W, k, s)
    r = _f16(u((B, Ho, Wo, cout), -0.5, 0.5)) if res else None
    return x, w, alpha, beta, r


def _standin(x, w, alpha, beta, r, s, variant="correct"):
    """The F16 conv as a kernel computes it, torch's fp32 convolution standing in for the MFMA chain: fp32 accumulate, fp32 epilogue, one
    rounding to fp16 -- or a wrong epilogue.  Returns fp32 [M, cout] holding fp16 values."""
    cout, k = w.shape[0], w.shape[2]
    acc = F.conv2d(x.permute(0, 3, 1, 2), w, None, s, (k - 1) // 2).permute(0, 2, 3, 1).reshape(-1, cout)
    b = _f16(beta) if variant == "f16 beta" else beta
    v = (acc * alpha if alpha is not None else acc) + b
    slope = float(_f16(torch.tensor(0.1))) if variant == "f16 slope" else 0.1
    v = torch.where(v > 0, v, torch.tensor(slope, dtype=torch.float32) * v)
    if variant == "rounding before the residual add":
        v = _f16(v)
    if r is not None:
        v = v + r.reshape(-1, cout)
    if variant == "truncation":                            # the 13 low bits of the fp32 value dropped (normal range here)
        return (v.view(torch.int32) & -8192).view(torch.float32)
    return _f16(v)


def _judge(case, seed, variant):
    cin, cout, k, s, B, H, W, res, alpha_none = case
    x, w, alpha, beta, r = _operands(cin, cout, k, s, B, H, W, res, alpha_none, seed)
    ref = cr.conv_desc_ref(x, w, beta, alpha, r, stride=s)
    mag = cr.conv_desc_mag(x, w, beta, alpha, r, stride=s)
    return _standin(x, w, alpha, beta, r, s, variant), ref, mag, k * k * cin


@pytest.mark.parametrize("case", BF16_SHAPES, ids=["%d-%d k%d s%d%s%s" % (c[0], c[1], c[2], c[3], " res" * c[7], " alphaNULL" * c[8])
                                                   for c in BF16_SHAPES])
def test_f16_bar_passes_a_correct_fp32_accumulated_conv(case):
    """The six shapes of the BF16 bar's pin with fp16 operands, seed 7: no element outside its interval, share at most a quarter of the
    cap (7.4e-4 .. 4.5e-3 measured, the largest at K = 4608)."""
    got, ref, mag, K = _judge(case, 7, "correct")
    r = cf.assert_f16(got, ref, mag, K, "torch fp32 stand-in %s" % (case,))
    print("f16 bar | stand-in %s | worst |d|/eps %.4g | share %.3g" % (case, r["worst"], r["share"]))
    assert r["share"] <= cf.F16_SHARE_CAP / 4, r


@pytest.mark.parametrize("variant", ["truncation", "f16 beta", "f16 slope", "rounding before the residual add"])
def test_f16_bar_catches_wrong_epilogues(variant):
    """512->256 3x3 at 2 x 13 x 13 (K = 4608; with a residual for the rounding before the add, which needs one).  Every variant fails B
    with a share of at least 4x the cap (truncation 0.50, beta held in fp16 0.205, LeakyReLU slope held in fp16 0.18); truncation and the
    fp16 beta fail A too (so does the early rounding here; the slope's error is relative to a small negative output and stays inside
    eps: only B sees it)."""
    case = (512, 256, 3, 1, 2, 13, 13, variant == "rounding before the residual add", False)
    got, ref, mag, K = _judge(case, 11, variant)
    r = cf.f16_report(got, ref, mag, K)
    print("f16 bar | %s | share %.3g | outside %d" % (variant, r["share"], r["outside"]))
    assert not r["b_ok"] and r["share"] >= 4 * cf.F16_SHARE_CAP, r
    with pytest.raises(AssertionError, match="criterion"):
        cf.assert_f16(got, ref, mag, K, variant)
    if variant in ("truncation", "f16 beta"):
        assert not r["a_ok"] and r["first"] is not None, r
        with pytest.raises(AssertionError, match="criterion A"):
            cf.assert_f16(got, ref, mag, K, variant)
    ok = cf.f16_report(_judge(case, 11, "correct")[0], ref, mag, K)
    assert ok["a_ok"] and ok["b_ok"], ok


# ----------------------------------------------------------------------------- selection: an F16 descriptor takes the BF16 descriptor's choice
def _bf16_points():
    for cfg, (dtype, _, _, _) in grid.ALL_CONFIGS.items():
        if dtype != grid.BF16:
            continue
        if cfg in grid.CONFIGS:
            pts = [(size, B) for size in grid.SIZES for B in grid.BATCHES]
        else:
            pts = grid.MORE_POINTS.get(cfg, (grid.POINT[grid.BF16],))
        for size, B in pts:
            yield cfg, size, B


def test_f16_descriptor_takes_the_bf16_choice():
    """Every distinct layer of the network at 416 and 608, the grid's batch sizes, every BF16 configuration of the selection table
    (defaults, YV3_OPT_K3S1, forced codes 1, 5-9, 11, 13-16, the tune bits, big_tile_min, no ping-pong): yv3_conv2d_form, _launches
    and _kernel answer for the F16 descriptor what they answer for the BF16 one -- on the host selector's 256 CUs, nothing launched."""
    lib = _ffi.lib()
    per_size = {size: grid.classes(size)[0] for size in grid.SIZES}
    n, diff = 0, []                                       # (n: answered with a choice; the 3-channel first layer is YV3_ESHAPE for both)
    for cfg, size, B in _bf16_points():
        for i, layer in enumerate(per_size[size]):
            d = grid.make_desc(lib, cfg, size, B, layer)
            want = grid.query(lib, d)
            d.dtype = _ffi.F16
            if d.out_dtype != _ffi.F32:
                d.out_dtype = _ffi.F16
            got = grid.query(lib, d)
            n += want[0] >= 0
            if got != want or (want[0] < 0) != (i == 0):
                diff.append("%s/%d/%d distinct layer %d: F16 %s, BF16 %s" % (cfg, size, B, i, got, want))
    assert n > 1000
    assert not diff, "%d differences, first:\n%s" % (len(diff), "\n".join(diff[:20]))


def test_f16_descriptor_error_contract_on_the_host():
    """The invalid descriptors of the error-contract test answer the plane modes' codes for dtype F16; code 4 (the Python side's BF16_ACT)
    and code 7 stay unknown dtypes."""
    from tests.test_gpu_conv_matrix import ERROR_CASES
    lib = _ffi.lib()
    ptrs = {"x": grid.PTR, "x2": grid.PTR + 0x100, "w": grid.PTR + 0x200, "beta": grid.PTR + 0x300, "dec": grid.PTR + 0x400, "other": _ffi.F32H2}

    def base(dtype):
        d = _ffi.ConvDesc()
        d.x, d.w, d.beta, d.y, d.flags = ptrs["x"], ptrs["w"], ptrs["beta"], grid.PTR + 0x500, grid.PTR + 0x600
        d.B, d.H, d.W, d.cin, d.cout, d.cout_pad, d.k, d.stride = 1, 4, 4, 64, 64, 64, 1, 1
        d.act, d.dtype, d.out_dtype = _ffi.ACT_LEAKY, dtype, dtype
        return d
    assert grid.query(lib, base(_ffi.F16))[:2] == (0, 1)
    for name, mutate, _, want in ERROR_CASES:
        if want is None or name.startswith("y NULL"):
            continue
        d = base(_ffi.F16)
        mutate(d, ptrs)
        assert grid.query(lib, d) == (want, want, want), name
    for code in (_ffi.BF16_ACT, 7):
        assert grid.query(lib, base(code)) == (-4, -4, -4)


def test_mode_code_equals_the_header():
    import yolo_v3_amd
    with open(os.path.join(REPO, "include", "yv3.h")) as f:
        m = re.search(r"^#define\s+YV3_F16\s+(\d+)", f.read(), re.M)
    assert m and int(m.group(1)) == yolo_v3_amd.F16 == _ffi.F16 == 5
    from yolo_v3_amd import engine
    assert engine.PLANES[_ffi.F16] == 1 and engine._TORCH_DTYPE[_ffi.F16] == torch.float16
    assert engine.RANGE_FALLBACK[_ffi.F16] == _ffi.BF16 and engine.RANGE_FALLBACK[_ffi.F32H2] == _ffi.F32X3
    from yolo_v3_amd.detect import two_lanes_min_pixels
    assert two_lanes_min_pixels(_ffi.F16) == two_lanes_min_pixels(_ffi.BF16)


def test_pack_conv_weight_accepts_f16_for_k1_and_k3_only():
    """The argument checks run before any launch: a NULL output answers YV3_EINVAL for every dtype, k = 4 (Winograd filters) YV3_ESHAPE
    for F16, which has no Winograd form."""
    lib = _ffi.lib()
    assert lib.yv3_pack_conv_weight(grid.PTR, None, 64, 64, 3, 64, _ffi.F16, None) == _ffi.EINVAL
    assert lib.yv3_pack_conv_weight(grid.PTR, grid.PTR, 64, 64, 4, 64, _ffi.F16, None) == _ffi.ESHAPE
    assert lib.yv3_split_plane_f16(None, grid.PTR, 8, None) == _ffi.EINVAL and lib.yv3_merge_plane_f16(grid.PTR, None, 8, None) == _ffi.EINVAL
    assert lib.yv3_split_plane_f16(grid.PTR, grid.PTR, 0, None) == 0 and lib.yv3_merge_plane_f16(grid.PTR, grid.PTR, 0, None) == 0


def test_backprop_math_f16_is_rejected_before_anything_runs():
    from yolo_v3_amd import YoloNet, F16, Yv3Error, backprop
    net = YoloNet((96, 96), numClass=3)
    net.backprop_math = F16
    with pytest.raises(Yv3Error) as e:
        backprop.backprop_math(net)
    assert e.value.code == _ffi.EINVAL
    net.backprop = True
    with pytest.raises(Yv3Error) as e:                    # the training entry point itself: CPU tensors, nothing packed, nothing launched
        net(torch.zeros(1, 3, 96, 96), torch.zeros(1, 1, 5))
    assert e.value.code == _ffi.EINVAL


# ----------------------------------------------------------------------------- the definition on the CPU
# Relative L2 error of the three head-logit maps against the fp32 oracle, 416x416, synth.images(1, 416, 2006), as the mode was proposed:
# oracle_cpu's prec="bf16" trunk with its rounding function swapped for fp16 (RECORDED_F16; prec="bf16" as it is: RECORDED_BF16).  The
# test repeats that measurement itself (`hooked`, same process, same thread setting) and holds tests/f16_ref.py to it.
RECORDED_F16 = {"SW-1": (1.04e-3, 1.02e-3, 9.4e-4), "trained-like": (7.9e-4, 6.6e-4, 3.3e-4)}
RECORDED_BF16 = {"SW-1": (8.1e-3, 8.5e-3, 8.2e-3), "trained-like": (6.4e-3, 5.4e-3, 2.6e-3)}
MAX_STORED = {"SW-1": 33.0, "trained-like": 88.0}


@pytest.mark.parametrize("weights", ["SW-1", "trained-like"])
def test_f16_ref_reproduces_the_hooked_oracle(weights, monkeypatch):
    """tests/f16_ref.py without its weight scale IS the hooked oracle (the same torch ops in the same order): its three errors equal the
    hooked oracle's to 3 digits -- in fact the logits are equal bit for bit.  The definition itself, with the per-channel power-of-two
    weight scale, differs from that only in the weights that are fp16 subnormals unscaled (SW-1: 88 823 of them, 3 001 after the scale);
    every stored rounding that this flips moves everything downstream, so its errors are printed beside the others, and held to 1/8 of the
    bf16 definition's like them."""
    stream = synth.weight_stream() if weights == "SW-1" else helpers.trained_like_stream()
    sd, _ = oc.state_dict_from_stream(stream)
    x = torch.from_numpy(synth.images(1, 416, 2006))
    with torch.no_grad():
        ref = oc.head_logits(sd, x)
        stats = {}
        got = f16_ref.head_logits(sd, x, stats)
        plain = f16_ref.head_logits(sd, x, scale=False)
        monkeypatch.setattr(oc, "round_bf16", lambda t: t.half().float())
        hooked = oc.head_logits(sd, x, prec="bf16")
        monkeypatch.undo()
    errs, e_plain, e_hooked = ([f16_ref.rel_l2(a, b) for a, b in zip(t, ref)] for t in (got, plain, hooked))
    fmt = lambda v: " / ".join("%.4g" % e for e in v)
    print("f16_ref | %s | relative L2 of the head logits: hooked oracle %s | f16_ref without the weight scale %s | the definition %s | "
          "recorded %s | largest stored activation %.4g" % (weights, fmt(e_hooked), fmt(e_plain), fmt(errs), fmt(RECORDED_F16[weights]),
                                                          stats["max_stored"]))
    for a, b in zip(e_plain, e_hooked):
        assert abs(a - b) <= 5e-4 * b, (e_plain, e_hooked)                 # 3 digits
    assert all(torch.equal(a, b) for a, b in zip(plain, hooked))
    for e, h, bf in zip(errs, e_hooked, RECORDED_BF16[weights]):
        assert 0.1 <= e / bf <= 0.15 and 0.1 <= h / bf <= 0.15             # 2^-11 / 2^-8 = 1/8 of the bf16 definition's error
    assert abs(stats["max_stored"] - MAX_STORED[weights]) <= 1.0 and stats["max_stored"] < cf.F16_MAX
