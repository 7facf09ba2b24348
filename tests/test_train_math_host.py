"""The table of the training step's math modes (yolo_v3_amd/backprop.py: MATH, one _Math per net.backprop_math) against the
library's export list (yolo_v3_amd/_ffi.py).  No GPU and no library: the table names its entry points."""
import inspect
import re

from yolo_v3_amd import _ffi, backprop, F32, BF16, BF16_ACT

TRAIN_EXPORTS = {n for n in _ffi.EXPORTS if n.startswith("yv3_train_")}
COMMON_ENTRIES = {"yv3_train_add", "yv3_train_upcat_bwd", "yv3_train_bn_eval_stats", "yv3_train_to_bf16"}     # the same in every mode


def entry_points(m):
    return {getattr(m, f) for f in backprop.ENTRIES}

# the fields that carry the kernels of the activation's dtype: what BF16_ACT changes in BF16
ACT_FIELDS = {"conv_fwd", "channel_ws", "bn_stats", "bn_act_fwd", "bn_act_bwd", "bias_bwd"}


def test_one_record_per_math_mode():
    assert set(backprop.MATH) == {F32, BF16, BF16_ACT}
    assert set(backprop.ENTRIES) < set(backprop._Math._fields) and len(backprop.ENTRIES) == 12


def test_every_entry_point_is_exported():
    for math, m in backprop.MATH.items():
        for f in backprop.ENTRIES:
            assert getattr(m, f) in TRAIN_EXPORTS, (math, f, getattr(m, f))
    assert COMMON_ENTRIES <= TRAIN_EXPORTS


def test_table_and_common_calls_cover_the_training_exports():
    source = inspect.getsource(backprop)
    called = set(re.findall(r'_call\(lib, "(yv3_train_\w+)"', source))           # the calls made by name, outside the table
    assert called == COMMON_ENTRIES, called
    used = set(COMMON_ENTRIES)
    for m in backprop.MATH.values():
        used |= entry_points(m)
    assert used == TRAIN_EXPORTS, (sorted(used - TRAIN_EXPORTS), sorted(TRAIN_EXPORTS - used))


def test_f32_names_no_bf16_entry_point():
    assert not [n for n in entry_points(backprop.MATH[F32]) if "_bf16" in n]


def test_bf16_act_differs_from_bf16_in_the_activation_kernels_only():
    a, b = backprop.MATH[BF16], backprop.MATH[BF16_ACT]
    assert {f for f in backprop.ENTRIES if getattr(a, f) != getattr(b, f)} == ACT_FIELDS
    assert ACT_FIELDS <= set(backprop.ENTRIES)


def test_adapted_entries_are_table_entries():
    named = set().union(*(entry_points(m) for m in backprop.MATH.values()))
    assert set(backprop._ADAPT) <= named


def test_twin_signatures_are_their_bases():
    twins = [n for n in TRAIN_EXPORTS if "_bf16" in n and n.replace("_bf16", "") in TRAIN_EXPORTS and not n.endswith("_bf16o")]
    assert len(twins) == 11, sorted(twins)
    for n in twins:
        res, args = _ffi._SIGNATURES[n]
        bres, bargs = _ffi._SIGNATURES[n.replace("_bf16", "")]
        assert res is bres and (args is bargs or list(args) == list(bargs)), n
