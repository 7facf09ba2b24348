"""The float64 training-step restatement (tests/train_ref.py) against one step of the reference's own YoloNet in .train() and .eval()
(tests/golden/train_step.npz, from tools/make_golden_train.py).  CPU only.

The fixture is the reference's fp32 CPU arithmetic; the bars below are a few times the difference that arithmetic leaves against
float64 on this case (see BARS)."""
import os
import zlib

import numpy as np
import pytest
import torch

from tests import train_ref as T
from tests import yolo_loss_ref as R
from tests.helpers import trained_like_stream

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_step.npz")
CASE = dict(size=96, B=2, C=3, T=8, image_seed=31, target_seed=53)
N_ENTRIES = 32


def entries(name, n):
    """The 32 seeded flat indices of a conv weight gradient stored in the fixture."""
    g = np.random.default_rng(zlib.crc32(name.encode()))
    return np.sort(g.choice(n, size=min(N_ENTRIES, n), replace=False))


def put16(arrays, key, tensors):
    """Store a list of tensors as one flat fp16 array, each tensor times its own power of two chosen so that its max|a| lands in
    [2^13, 2^14): every element at least 2^-28 of the maximum keeps fp16's 11-bit significand (relative error <= 2^-11), smaller ones
    add nothing to a relative L2 norm."""
    parts, exps = [], []
    for a in tensors:
        a = np.asarray(a, np.float64).ravel()
        m = float(np.abs(a).max()) if a.size else 0.0
        e = int(np.floor(np.log2(m))) - 13 if m > 0 else 0
        parts.append((a * 2.0 ** -e).astype(np.float16))
        exps.append(e)
    arrays[key + "/h16"] = np.concatenate(parts)
    arrays[key + "/exp"] = np.array(exps, np.int32)


def get16(gold, key, shapes):
    """The tensors put16 stored under `key`, as float64 arrays of `shapes`."""
    flat, exps, out, p = gold[key + "/h16"], gold[key + "/exp"], [], 0
    assert len(exps) == len(shapes)
    for sh, e in zip(shapes, exps):
        n = int(np.prod(sh))
        out.append(flat[p:p + n].astype(np.float64).reshape(sh) * 2.0 ** int(e))
        p += n
    assert p == flat.size
    return out


def running_keys(sd):
    return [k for k in sd if k.endswith(("running_mean", "running_var"))]


def state_dict():
    from yolo_v3_amd import YoloNet, WeightManager
    net = YoloNet((CASE["size"], CASE["size"]), numClass=CASE["C"])
    WeightManager(net).load_stream(trained_like_stream(CASE["C"]))
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def case():
    """(state_dict, x, target, attempt): the first target draw whose decisions clear the 1e-4 margins in both modes."""
    from yolo_v3_amd import synth
    sd = state_dict()
    x = synth.images(CASE["B"], CASE["size"], CASE["image_seed"])
    lg = [T.forward(sd, x, train)[0] for train in (True, False)]
    for attempt in range(100):
        tg = R.random_rows(CASE["target_seed"] * 1000 + attempt, CASE["B"], CASE["T"], CASE["C"], (0.05, 0.7))
        if all(R.margins_ok(r["margins"]) for l in lg for r in T.head_losses(l, tg, CASE["size"], CASE["C"])):
            return sd, x, tg, attempt
    raise AssertionError("no target draw clears the margins")


@pytest.fixture(scope="module")
def fixture_case():
    gold = np.load(GOLD)
    sd, x, tg, attempt = case()
    assert attempt == int(gold["attempt"]) and np.array_equal(tg, gold["target"])
    return gold, sd, x, tg


LOSS_BAR = 1e-5        # loss and stats, relative
# Gradient bars, ~3-10x the distance between the reference's fp32 step and float64 measured on this case.  In .train() that distance is
# large (up to 3e-3 relative L2 on a BN gradient): 96x96 at bs=2 leaves 18 samples per channel in the 3x3 head's BatchNorm, where
# fp32 rounding in the batch statistics and the LeakyReLU kink are amplified; in .eval() it is ~1e-6.  The BN / bias gradients and the
# running statistics' change are stored in fp16 (put16: <= 2^-11 = 4.9e-4 relative L2), so their .eval() bar is that storage error
# (2x); the conv-weight sums and entries are stored in fp32 / fp64 and keep the tight bars.
#            rel L2 of BN / bias grads and running stats, |sum - ref| / (sqrt(sumsq) sqrt(n)), sumsq relative, entries / sqrt(sumsq)
BARS = dict(train=dict(vec=1e-2, sum=1e-3, sumsq=1e-2, entries=4e-3),
            eval=dict(vec=1e-3, sum=1e-6, sumsq=1e-5, entries=1e-6))


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_restatement_matches_the_reference_step(fixture_case, mode):
    gold, sd, x, tg = fixture_case
    out = T.run(sd, x, tg, CASE["C"], train=mode == "train")
    bar = BARS[mode]
    assert abs(out["loss"] - float(gold[mode + "/loss"])) <= LOSS_BAR * abs(float(gold[mode + "/loss"]))
    st = np.array(out["stats"], np.float64)
    ref = gold[mode + "/stats"]
    assert np.all(np.abs(st - ref) <= LOSS_BAR * np.maximum(np.abs(ref), 1.0))
    rk = running_keys(sd)
    got_run = {"%s.bn.%s" % (p, n): t for p, (m, v) in out["running"].items() for n, t in (("running_mean", m), ("running_var", v))}
    assert sorted(got_run) == sorted(rk)
    deltas = get16(gold, "train/running_delta", [tuple(sd[k].shape) for k in rk]) if mode == "train" else None
    for i, k in enumerate(rk):
        before = sd[k].double()
        if mode == "train":
            ref_run = before + torch.from_numpy(deltas[i])
            assert T.rel_l2(got_run[k], ref_run) <= bar["vec"], k
            assert T.rel_l2(got_run[k] - before, ref_run - before) <= bar["vec"], k
        else:
            assert torch.equal(got_run[k], before), k
    conv = [k for k, g in out["grads"].items() if g.dim() == 4]
    vec = [k for k, g in out["grads"].items() if g.dim() != 4]
    sums, ents = gold[mode + "/conv_sums"], gold[mode + "/conv_entries"]
    for i, k in enumerate(conv):
        g = out["grads"][k].double()
        s, ss = sums[i]
        scale = np.sqrt(ss)
        assert abs(float(g.sum()) - s) <= bar["sum"] * scale * np.sqrt(g.numel()), k
        assert abs(float((g * g).sum()) - ss) <= bar["sumsq"] * ss, k
        ent = g.reshape(-1)[torch.from_numpy(entries(k, g.numel()))]
        assert float((ent - torch.from_numpy(ents[i]).double()).abs().max()) <= bar["entries"] * scale, k
    for k, ref in zip(vec, get16(gold, mode + "/vec_grads", [tuple(out["grads"][k].shape) for k in vec])):
        assert T.rel_l2(out["grads"][k], ref) <= bar["vec"], k
    n_conv = len(conv)
    assert n_conv == 75
