"""engine.MODES without a GPU: what the table says of each inference math mode, pinned as literals -- the values the engine, the plans
and the detector had spread over their code before the table -- so that a record cannot drift silently."""
import importlib
import types

import pytest
import torch

from yolo_v3_amd import _ffi, arch, engine, YoloNet
from yolo_v3_amd._ffi import F32, BF16, F32X3, F32H2, F16, I8

detect = importlib.import_module("yolo_v3_amd.detect")          # (the package exports the function detect under this name)
SIX = (F32, BF16, F32X3, F32H2, F16, I8)

OVERFLOW_F32H2 = ("an activation exceeded the fp16 range (|v| > 65504) and was saturated: math mode F32H2 cannot "
                  "represent this network/input; set net.math_mode = yolo_v3_amd.F32X3 (or F32) and rerun "
                  "(net.strict_range = False, the default, does that by itself)")
OVERFLOW_F16 = ("an activation exceeded the fp16 range (|v| > 65504) and was saturated: math mode F16 cannot represent this "
                "network/input; set net.math_mode = yolo_v3_amd.BF16 (the same cost, fp32's exponent range, 8 bits) or F32X3 / F32 "
                "and rerun (net.strict_range = False, the default, re-runs in BF16 by itself)")
OVERFLOW_BF16 = ("the first layer of math mode BF16 runs on the fp16 matrix cores and needs |input| <= 4094 and "
                 "|weight| <= 255 (csrc/conv0.hip); this input / these weights exceed that and were saturated: "
                 "use net.math_mode = yolo_v3_amd.F32X3 (or F32)")
OVERFLOW = {F32H2: OVERFLOW_F32H2, F32X3: OVERFLOW_F32H2, F32: OVERFLOW_F32H2, BF16: OVERFLOW_BF16, I8: OVERFLOW_BF16, F16: OVERFLOW_F16}
FALLBACK_WARNING = {
    F32H2: "yolo_v3_amd: an activation left the fp16 range of math mode F32H2 (|v| > 65504); this network now runs in F32X3 (three bf16 "
           "planes: fp32 range, 24 bits, ~1.9x the time) -- set net.math_mode = F32X3 / F32 to avoid the first, discarded pass, or "
           "net.strict_range = True to get an error instead",
    F16: "yolo_v3_amd: an activation left the fp16 range of math mode F16 (|v| > 65504); this network now runs in BF16 (one bf16 plane: "
         "fp32 range, 8 bits instead of 11, the same time) -- set net.math_mode = BF16 to avoid the first, discarded pass, or "
         "net.strict_range = True to get an error instead"}


@pytest.fixture(scope="module")
def net():
    return YoloNet((416, 416)).eval()


def test_the_six_modes_and_the_names_derived_from_them():
    assert set(engine.MODES) == set(SIX) and [engine.MODES[c].name for c in SIX] == ["F32", "BF16", "F32X3", "F32H2", "F16", "I8"]
    assert engine.PLANES == {F32: 0, BF16: 1, F32X3: 3, F32H2: 2, F16: 1, I8: 1}
    assert engine._TORCH_DTYPE == {F32: torch.float32, BF16: torch.bfloat16, F32X3: torch.bfloat16, F32H2: torch.float16,
                                   F16: torch.float16, I8: torch.int8}
    assert engine.RANGE_FALLBACK == {F32H2: F32X3, F16: BF16}
    assert detect.TWO_LANES_MIN_IMAGES_416 == {F32H2: 40, F32X3: 40, F32: 52, BF16: 120, F16: 120, I8: 120}
    assert detect.two_lanes_min_pixels(F32) == 52 * 416 * 416 and detect.two_lanes_min_pixels(99) == 40 * 416 * 416 == detect.TWO_LANES_MIN_PIXELS
    assert {c: m.launch for c, m in engine.MODES.items()} == {F32: F32, BF16: BF16, F32X3: F32X3, F32H2: F32H2, F16: F16, I8: BF16}
    assert [c for c, m in engine.MODES.items() if m.mixed] == [I8] and engine.I8_FIRST == 4
    assert engine.Engine.OVERFLOW_MSG == OVERFLOW_F32H2


def test_plan_facts():
    """What Plan and Engine.checks_status branched on, mode by mode."""
    M = engine.MODES
    assert {c for c in SIX if M[c].head_decode} == {BF16, F32X3, F32H2, F16, I8}                # (was: dt != F32)
    assert {c for c in SIX if M[c].front is not None} == {F32H2, BF16, F32, F16, I8}
    assert {c for c in SIX if not M[c].front_optional} == {I8}
    assert engine._ADAPT == {"yv3_split_plane_f16": 3, "yv3_merge_plane_f16": 3, "yv3_conv_front_f32": 11, "yv3_res_block64_f32": 11}
    assert {c for c in SIX if M[c].stream_k} == {F32H2} == {c for c in SIX if M[c].batch_split}
    assert {c for c in SIX if M[c].always_status} == {F32H2, BF16, F16, I8}
    assert {c for c in SIX if M[c].wino4} == {F32}
    assert {c for c in SIX if M[c].row_scale} == {F32H2, F16}
    assert {c: (M[c].front, M[c].res64) for c in SIX if M[c].front} == {
        F32: ("yv3_conv_front_f32", "yv3_res_block64_f32"), F32H2: ("yv3_conv_front", "yv3_res_block64"),
        BF16: ("yv3_conv_front_bf16", "yv3_res_block64_bf16"), F16: ("yv3_conv_front_f16", "yv3_res_block64_f16"),
        I8: ("yv3_conv_front_bf16", "yv3_res_block64_bf16")}
    assert {c: (M[c].split, M[c].merge) for c in SIX} == {
        F32: (None, None), I8: (None, None), F16: ("yv3_split_plane_f16", "yv3_merge_plane_f16"),
        BF16: ("yv3_split_planes", "yv3_merge_planes"), F32X3: ("yv3_split_planes", "yv3_merge_planes"), F32H2: ("yv3_split_planes", "yv3_merge_planes")}


def test_every_entry_point_exists_in_the_library():
    lib = _ffi.lib()
    for c, m in engine.MODES.items():
        names = [v for v in m if isinstance(v, str) and v.startswith("yv3_")]
        assert len(names) == {F32: 2, BF16: 4, F32X3: 2, F32H2: 4, F16: 4, I8: 2}[c], (m.name, names)
        for n in names:
            assert hasattr(lib, n), (m.name, n)
    # an adapted entry point has its field's other entries' arguments but the one engine.entry drops
    for n, like in (("yv3_split_plane_f16", "yv3_split_planes"), ("yv3_merge_plane_f16", "yv3_merge_planes"),
                    ("yv3_conv_front_f32", "yv3_conv_front"), ("yv3_res_block64_f32", "yv3_res_block64")):
        full, i = list(getattr(lib, like).argtypes), engine._ADAPT[n]
        assert list(getattr(lib, n).argtypes) == full[:i] + full[i + 1:], n
    assert engine.entry("yv3_conv_front") is lib.yv3_conv_front


def test_wino_eligible_is_the_rule_it_was():
    def rule(sp, dtype):
        if not (sp.k == 3 and sp.stride == 1 and sp.bn):
            return False
        if dtype == F32H2:
            return sp.cin >= 256
        return dtype == F32 and sp.cin >= 64 and sp.cout % 128 == 0
    specs = arch.conv_specs(80)
    for c in SIX:
        got = [engine.wino_eligible(sp, c) for sp in specs]
        assert got == [rule(sp, c) for sp in specs], engine.MODES[c].name
    assert sum(engine.wino_eligible(sp, F32H2) for sp in specs) > 0 and sum(engine.wino_eligible(sp, F32) for sp in specs) == 31


def test_cout_pad_rule():
    for c in SIX:
        assert [engine.conv_cout_pad(n, c) for n in (18, 128, 135)] == ([32, 128, 160] if c == F32 else [32, 128, 256]), engine.MODES[c].name


def test_no_layout_conversion_for_i8():
    for f in (engine.to_planes, engine.from_planes):
        with pytest.raises(_ffi.Yv3Error) as e:
            f(torch.zeros(1, 2, 2, 4), I8)
        assert str(e.value) == "an int8 tensor is integers and a scale: there is no layout conversion for I8"
    x = torch.rand(1, 2, 2, 4)
    assert torch.equal(engine.to_planes(x, F32), x) and engine.from_planes(x, F32) is x


def test_engine_accepts_the_six_modes_only(net):
    for c in SIX:
        eng = engine.Engine(net, c)
        assert eng.mode is engine.MODES[c] and eng.dtype == c
    for bad in (4, 7, -1, True):
        with pytest.raises(_ffi.Yv3Error) as e:
            engine.Engine(net, bad)
        assert e.value.code == _ffi.EINVAL and all(n in str(e.value) for n in ("F32", "BF16", "F32X3", "F32H2", "F16", "I8")) and repr(bad) in str(e.value)
    with pytest.raises(_ffi.Yv3Error) as e:
        engine.Engine(net, I8, n_conv=74)
    assert str(e.value) == "I8 is an inference mode of the whole network: there is no int8 prefix engine"
    assert engine.Engine(net, BF16, n_conv=74).n_conv == 74
    net.math_mode = 4                     # the net takes anything: the error comes when an engine is asked for
    try:
        with pytest.raises(_ffi.Yv3Error):
            net.engine()
    finally:
        net.math_mode = F32H2
        net._engines.pop(4, None)


def test_checks_status(net):
    for c in SIX:
        assert engine.Engine(net, c).checks_status() == (c != F32X3), engine.MODES[c].name           # (F32: F(4x4) may use the even schedule)
    eng = engine.Engine(net, F32)
    for attr in ("winograd", "winograd4"):
        setattr(eng, attr, False)
        assert not eng.checks_status()
        setattr(eng, attr, True)
    eng.stream_k = False
    assert not eng.checks_status()
    eng = engine.Engine(net, F32H2)
    eng.winograd, eng.stream_k = False, False
    assert eng.checks_status()


def test_overflow_messages(net):
    for c in SIX:
        plan = types.SimpleNamespace(flags=torch.ones(1, dtype=torch.int32), flags_host=torch.ones(1, dtype=torch.int32), flags_event=object())
        eng = engine.Engine(net, c)
        eng.raise_if_overflowed(plan, 0)
        assert int(plan.flags[0]) == 1
        with pytest.raises(engine.RangeOverflow) as e:
            eng.raise_if_overflowed(plan, 1)
        assert str(e.value) == OVERFLOW[c], engine.MODES[c].name
        assert int(plan.flags[0]) == 0 and int(plan.flags_host[0]) == 0 and plan.flags_event is None
        with pytest.raises(engine.StreamKTimeout):
            eng.raise_if_overflowed(plan, 3)


def test_range_fallback_warnings():
    for c in SIX:
        net = types.SimpleNamespace(numClass=80, anchors_flat=[1.0] * 18, strict_range=False)
        net.engine = lambda dtype, net=net: engine.Engine(net, dtype)
        eng = engine.Engine(net, c)
        if c not in FALLBACK_WARNING:
            assert eng.range_fallback() is None and "_range_fallback" not in net.__dict__
            continue
        with pytest.warns(RuntimeWarning) as rec:
            fb = eng.range_fallback()
        assert [str(w.message) for w in rec] == [FALLBACK_WARNING[c]]
        assert fb.dtype == {F32H2: F32X3, F16: BF16}[c] and net._range_fallback == {c: fb.dtype}
        net.strict_range = True
        assert eng.range_fallback() is None
