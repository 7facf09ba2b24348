"""The per-op float64 references of tests/train_kernel_ref.py, chained over YoloNet's graph as yolo_v3_amd/backprop.py chains the
kernels, against the autograd step of tests/train_ref.py / tests/train_ref_bf16.py on the case of tests/golden/train_step.npz
(tests/test_train_host.py pins train_ref to the reference's own step there).  The two are the same float64 arithmetic in different
orders, so they agree to float64 round-off; the bar leaves three decades over the 1e-13 .. 1e-12 a 75-layer chain accumulates.
CPU only."""
import pytest
import torch
import torch.nn.functional as F

from tests import test_train_host as H
from tests import train_kernel_ref as K
from tests import train_ref as T
from tests import train_ref_bf16 as TB

CHAIN_BAR = 1e-9


@pytest.fixture(scope="module")
def golden_case():
    from yolo_v3_amd import YoloNet
    sd, x, tg, _ = H.case()
    net = YoloNet((H.CASE["size"], H.CASE["size"]), numClass=H.CASE["C"])
    return net, sd, torch.from_numpy(x), tg


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("rounding", [False, True], ids=["f32", "bf16"])
def test_chained_per_op_references_reproduce_the_autograd_step(golden_case, train, rounding):
    net, sd, x, tg = golden_case
    C, size = H.CASE["C"], H.CASE["size"]
    ref = TB.run(sd, x, tg, C, train=train, rounding=rounding)

    def dlogits_of(logits):
        return [torch.from_numpy(r["grad"]) for r in T.head_losses(logits, tg, size, C)]

    out = K.chain_step(net, sd, x, dlogits_of, train=train, rounding=rounding)
    assert sorted(out["grads"]) == sorted(ref["grads"]) and len(out["grads"]) == 75 + 2 * 72 + 3
    worst = max(T.rel_l2(out["grads"][k], g) for k, g in ref["grads"].items())
    for prefix, (m, v) in ref["running"].items():
        worst = max(worst, T.rel_l2(out["running"][prefix + ".bn"][0], m), T.rel_l2(out["running"][prefix + ".bn"][1], v))
    print("worst rel L2 of the chain against autograd: %.3g" % worst)
    assert worst <= CHAIN_BAR


def test_closed_form_bn_matches_autograd_and_torch_refuses_one_row():
    g = torch.Generator().manual_seed(5)
    P, C = 37, 6
    z = torch.randn(P, C, generator=g, dtype=torch.float64) * 3 + 1
    dy, res = torch.randn(P, C, generator=g, dtype=torch.float64), torch.randn(P, C, generator=g, dtype=torch.float64)
    gam, bet = torch.rand(C, generator=g, dtype=torch.float64) + 0.5, torch.rand(C, generator=g, dtype=torch.float64) - 0.5
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.1
    for train in (True, False):
        zz, ga, be = z.clone().requires_grad_(True), gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
        rm2, rv2 = rm.clone(), rv.clone()
        u = F.batch_norm(zz.t().unsqueeze(0), rm2, rv2, ga, be, training=train, momentum=K.MOMENTUM, eps=K.EPS)
        y = F.leaky_relu(u, K.SLOPE)[0].t() + res
        y.backward(dy)
        if train:
            mean, var, invstd = K.bn_batch_stats(z)
            nm, nv = K.bn_running(mean, var, P, rm, rv)
            assert torch.allclose(nm, rm2, rtol=1e-12, atol=0) and torch.allclose(nv, rv2, rtol=1e-12, atol=0)
        else:
            mean, invstd = K.bn_eval_stats(rm, rv)
        assert torch.allclose(K.bn_act_fwd(z, mean, invstd, gam, bet, res), y.detach(), rtol=1e-12, atol=1e-13)
        b = K.bn_act_bwd(z, dy, mean, invstd, gam, bet, train)
        assert b["share"] == 0.0 and float(b["S"].abs().max()) == 0.0
        assert torch.allclose(b["dz"], zz.grad, rtol=1e-10, atol=1e-13)
        assert torch.allclose(b["dgamma"], ga.grad, rtol=1e-12, atol=1e-13) and torch.allclose(b["dbeta"], be.grad, rtol=1e-12, atol=1e-13)
    with pytest.raises(ValueError):            # one value per channel: torch has no train-mode reference, the P = 1 case writes it out
        F.batch_norm(z[:1].t().unsqueeze(0), rm.clone(), rv.clone(), gam, bet, training=True)
    mean, var, invstd = K.bn_batch_stats(z[:1])
    assert torch.equal(mean, z[0]) and float(var.abs().max()) == 0.0
    nm, nv = K.bn_running(mean, var, 1, rm, rv)
    assert torch.allclose(nv, 0.9 * rv, rtol=1e-15, atol=0)
    assert float(K.bn_act_bwd(z[:1], dy[:1], mean, invstd, gam, bet, True)["dz"].abs().max()) == 0.0


def test_kink_rule_marks_and_prices_an_undecided_element():
    z = torch.tensor([[1.0, 2.0], [3.0, -1.0], [0.5, 0.25]], dtype=torch.float64)
    mean, invstd = torch.tensor([1.0, 0.0], dtype=torch.float64), torch.tensor([2.0, 1.0], dtype=torch.float64)
    gam, bet = torch.tensor([1.0, 2.0], dtype=torch.float64), torch.tensor([1.0 + 1e-7, 0.5], dtype=torch.float64)
    dy = torch.tensor([[1.0, 1.0], [1.0, 1.0], [-3.0, 1.0]], dtype=torch.float64)
    b = K.bn_act_bwd(z, dy, mean, invstd, gam, bet, False)          # element (2, 0): xhat = -1, u = 1e-7, within 4e-6 * 2
    assert b["und"].tolist() == [[False, False], [False, False], [True, False]]
    assert b["S"].tolist() == [pytest.approx(0.9 * 3.0), 0.0] and b["share"] == pytest.approx(1 / 6)
    wrong_side = b["dbeta"].clone()
    wrong_side[0] += 0.9 * 3.0                                      # the kernel taking the other side moves dbeta by 0.9 |dy|
    r = K.bn_bwd_ratios(b["dz"], b["dgamma"], wrong_side, b)
    assert r["dbeta"] <= 1.0 and r["dz"] == 0.0
    wrong_side[1] += 1e-3                                           # a decided channel has no such allowance
    assert K.bn_bwd_ratios(b["dz"], b["dgamma"], wrong_side, b)["dbeta"] > 1.0
