"""The kernels of the BF16_ACT training step (csrc/train_bf16.hip's bf16-output conv forward, csrc/train_bf16_act.hip) one call at a
time, against float64 on the device's own inputs (tests/train_kernel_ref.py).

* The conv forward shares its main loop with yv3_train_conv_fwd_bf16, so its output is that call's fp32 output rounded by
  ``tensor.to(torch.bfloat16)``, bit for bit.
* The rounding itself: calls whose fp32 result is known exactly (a pure cast, an identity BatchNorm) give torch's cast bit for bit,
  on ties, binade crossings, +-0, subnormals and +-inf; a NaN becomes 0x7fc0.
* Values.  fp32 outputs (mean, invstd, running statistics, dgamma, dbeta, dbias) keep the fp32 kernels' bar of
  tests/test_gpu_train_edges.py (BN_BAR of the largest value, the kink rule of tests/train_kernel_ref.py).  A bf16 output is one
  rounding of such a result: |out - ref| <= 2^-8 |ref| (bf16's unit roundoff) plus that same fp32 bar.  A store that truncated, or
  rounded twice, breaks the first term.  The two ill-conditioned inputs are held, as for the fp32 kernels, to BAR_FACTOR times the error
  of torch's fp32 CPU run of the same op (a bf16 output: plus its one rounding).

Every output buffer carries a canary past its end.  Each test prints its worst error / bar ratio (<= 1 passes)."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_kernel_ref as K
from tests.test_gpu_train_edges import bn_data, bn_reference, BAR_FACTOR, GRID_STRIDE
from yolo_v3_amd import _ffi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
U = 2.0 ** -8                       # bf16's unit roundoff (8 significand bits, round to nearest)


def _buf(n):
    return torch.full((n + CANARY,), float("nan"), device=DEV, dtype=torch.float32)


def _buf16(n):
    return torch.full((n + CANARY,), 0x1234, device=DEV, dtype=torch.int16)


def _ok(b, n):
    return bool((b[n:] == 0x1234).all()) if b.dtype == torch.int16 else bool(torch.isnan(b[n:]).all())


def _p(t):
    return t.data_ptr() if t is not None else None


def _bits(t):
    """The bf16 image of an fp32 CPU tensor as torch casts it (int16 bits)."""
    return t.float().cpu().to(torch.bfloat16).view(torch.int16)


def _val(b):
    """int16 bf16 bits (GPU) -> float64 values (CPU)."""
    return b.cpu().view(torch.bfloat16).double()


def _ws(P, C):
    nb = _ffi.lib().yv3_train_channel_bf16_workspace_bytes(P, C)
    assert nb > 0
    return torch.empty(nb, device=DEV, dtype=torch.uint8), nb


# ---------------------------------------------------------------- conv forward with a bf16 result
#        id            B  H   W   cin  cout k  st  extras
CONV_CASES = [
    ("2x2-ragged",     1, 13, 13, 64,  136, 3, 1, {}),                   # 128x128 tiles, M = 169 and N = 136 both ragged
    ("4x1-cout24",     1, 20, 20, 32,  24,  3, 1, {}),                   # N <= 64
    ("1x4-7x7",        1, 7,  7,  256, 512, 1, 1, {}),                   # M <= 64
    ("stride2-13to7",  2, 13, 13, 32,  72,  3, 2, {}),
    ("first-nchw",     1, 16, 24, 3,   32,  3, 1, dict(nchw=True)),
    ("upcat-8x8",      2, 8,  8,  96,  64,  1, 1, dict(cin_up=32)),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_fwd_bf16o_is_the_fp32_output_rounded(case):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    name, B, H, W, cin, cout, k, st, ex = case
    cu, nchw = ex.get("cin_up", 0), int(bool(ex.get("nchw")))
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    x32 = torch.randn(B, cin, H, W, generator=g)
    w32 = (torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)).contiguous().to(DEV)
    dev_in = lambda t: (t if nchw else t.permute(0, 2, 3, 1)).contiguous().to(torch.bfloat16).to(DEV)
    low = torch.randn(B, cu, H // 2, W // 2, generator=g) if cu else None
    xin, x2 = dev_in(x32[:, cu:]), (dev_in(low) if cu else None)
    nwp = (cout + 7) // 8 * 8 * cin * k * k
    wf = _buf16(nwp)
    _ffi.check(lib.yv3_train_pack_weight_bf16(w32.data_ptr(), wf.data_ptr(), None, cout, cin, k, s))
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    nz = B * Ho * Wo * cout
    z32, zb = _buf(nz), _buf16(nz)
    _ffi.check(lib.yv3_train_conv_fwd_bf16(xin.data_ptr(), _p(x2), wf.data_ptr(), None, z32.data_ptr(), B, H, W, cin, cu, cout, k, st,
                                           nchw, s))
    _ffi.check(lib.yv3_train_conv_fwd_bf16o(xin.data_ptr(), _p(x2), wf.data_ptr(), zb.data_ptr(), B, H, W, cin, cu, cout, k, st, nchw, s))
    torch.cuda.synchronize()
    assert _ok(z32, nz) and _ok(zb, nz)
    want = z32[:nz].to(torch.bfloat16).view(torch.int16)
    differing = int((zb[:nz] != want).sum())
    print("conv_fwd_bf16o %s: %d of %d elements differ from the rounded fp32 output" % (name, differing, nz))
    assert differing == 0
    # and the fp32 output is the convolution (so the comparison above is not between two empty results)
    xfull = torch.cat((F.interpolate(K.rb(low), scale_factor=2, mode="nearest"), K.rb(x32[:, cu:])), 1) if cu else K.rb(x32)
    z64, za = K.conv_fwd(xfull.double(), K.rb(w32.cpu()).double(), st)
    assert K.conv_ratio(z32[:nz].view(B, Ho, Wo, cout), z64.permute(0, 2, 3, 1), za.permute(0, 2, 3, 1)) <= 1.0


def test_conv_fwd_bf16o_error_codes():
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    buf = torch.zeros(1 << 16, device=DEV, dtype=torch.int16)
    p = buf.data_ptr()
    assert lib.yv3_train_conv_fwd_bf16o(p, None, p, p, 1, 8, 8, 8, 0, 12, 3, 1, 0, s) == _ffi.ESHAPE          # cout % 8
    assert lib.yv3_train_conv_fwd_bf16o(p, None, p, p, 1, 8, 8, 12, 0, 16, 3, 1, 0, s) == _ffi.ESHAPE         # cin % 8
    assert lib.yv3_train_conv_fwd_bf16o(p, None, p, p, 1, 8, 8, 16, 8, 16, 3, 1, 0, s) == _ffi.EINVAL         # cin_up without x2
    assert lib.yv3_train_conv_fwd_bf16o(p, None, p, None, 1, 8, 8, 8, 0, 16, 3, 1, 0, s) == _ffi.EINVAL
    assert lib.yv3_train_conv_fwd_bf16o(p, None, p, p, 1, 8, 8, 8, 0, 16, 5, 1, 0, s) == _ffi.ESHAPE
    torch.cuda.synchronize()
    assert not bool(buf.any())


# ---------------------------------------------------------------- the rounding itself, bit for bit
def hostile_values():
    """fp32 values on which roundings differ: ties in both directions, the step into the next binade, +-0, subnormals, +-inf, NaN,
    and every other bit pattern at random."""
    bits = [0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x3f818001, 0x3f817fff,      # ties to even (down, up), just off a tie
            0x3fff8000, 0x3fffffff, 0x407f8000, 0x7f7f8000, 0x7f7fffff,                  # round up into the next binade / to inf
            0x00000000, 0x80000000, 0x00008000, 0x00018000, 0x00007fff, 0x00008001, 0x007fffff, 0x00000001, 0x80000001,
            0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff]
    t = torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)
    rnd = torch.randint(-2 ** 31, 2 ** 31, (4000,), generator=torch.Generator().manual_seed(5), dtype=torch.int64)
    return torch.cat([t, -t, rnd.to(torch.int32).view(torch.float32), torch.randn(4000, generator=torch.Generator().manual_seed(6))])


def test_bias_bwd_bf16_without_scale_is_torchs_cast():
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    C, ld = 255, 256
    v = hostile_values()
    P = (v.numel() + C - 1) // C
    dy = torch.zeros(P * C)
    dy[:v.numel()] = v
    dy = dy.view(P, C)
    ws, nb = _ws(P, C)
    dz, db = _buf16(P * ld), _buf(C)
    dyd = dy.to(DEV)
    assert torch.equal(dyd.cpu().view(torch.int32), dy.view(torch.int32))
    _ffi.check(lib.yv3_train_bias_bwd_bf16(dyd.data_ptr(), None, dz.data_ptr(), db.data_ptr(), P, C, ws.data_ptr(), nb, s))
    torch.cuda.synchronize()
    assert _ok(dz, P * ld) and _ok(db, C)
    got = dz[:P * ld].view(P, ld).cpu()
    want = _bits(dy)
    nan = torch.isnan(dy)
    assert nan.sum() > 10
    want[nan] = 0x7fc0              # (torch's own casts disagree on a NaN's bits -- scalar 0x7fc0, vectorised 0xffff; the kernels' is fixed)
    assert torch.equal(got[:, :C], want), dy[got[:, :C] != want][:8]
    assert bool((got[:, C:] == 0).all())


@pytest.mark.parametrize("P", [1, 338, 2 * 52 * 52])
@pytest.mark.parametrize("C", [18, 255])
@pytest.mark.parametrize("scale", [None, -1.75], ids=["noscale", "negative"])
def test_bias_bwd_bf16_values(scale, C, P):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    ld = (C + 7) // 8 * 8
    dl = torch.randn(P, C, generator=torch.Generator().manual_seed(P * 3 + C))
    sd_ = torch.tensor(scale, dtype=torch.float32, device=DEV) if scale is not None else None
    ws, nb = _ws(P, C)
    dz, db = _buf16(P * ld), _buf(C)
    dld = dl.to(DEV)
    assert lib.yv3_train_bias_bwd_bf16(dld.data_ptr(), _p(sd_), dz.data_ptr(), db.data_ptr(), P, C, ws.data_ptr(), nb - 1, s) == _ffi.EWORKSPACE
    _ffi.check(lib.yv3_train_bias_bwd_bf16(dld.data_ptr(), _p(sd_), dz.data_ptr(), db.data_ptr(), P, C, ws.data_ptr(), nb, s))
    torch.cuda.synchronize()
    assert _ok(dz, P * ld) and _ok(db, C)
    rd, rb_, ra = K.bias_bwd(dl.double(), scale)
    got = dz[:P * ld].view(P, ld).cpu()
    assert torch.equal(got[:, :C], _bits(rd.float())) and bool((got[:, C:] == 0).all())     # one fp32 multiply, one rounding
    worst = K.ratio(db[:C], rb_, K.BN_BAR * ra + 1e-30)                                     # dbias sums the fp32 products
    print("bias_bwd_bf16 P=%d C=%d scale=%s: worst error / bar %.3g" % (P, C, scale, worst))
    assert worst <= 1.0


def test_identity_bn_act_bwd_is_the_rounding_of_dy():
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    P, C = 37, 24
    g = torch.Generator().manual_seed(8)
    v = hostile_values()
    v = v[torch.isfinite(v)]
    dy = torch.randn(P * C, generator=g)
    dy[:min(v.numel(), 600)] = v[:600]
    z = (torch.rand(P, C, generator=g) + 0.5).to(torch.bfloat16).to(DEV)                    # positive: u = z > 0, du = dy
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    ws, nb = _ws(P, C)
    dz, dg, dbt = _buf16(P * C), _buf(C), _buf(C)
    dyd = dy.to(DEV)
    _ffi.check(lib.yv3_train_bn_act_bwd_bf16(z.data_ptr(), dyd.data_ptr(), zero.data_ptr(), one.data_ptr(), one.data_ptr(), zero.data_ptr(),
                                             dz.data_ptr(), dg.data_ptr(), dbt.data_ptr(), P, C, 0, ws.data_ptr(), nb, s))
    torch.cuda.synchronize()
    assert _ok(dz, P * C) and _ok(dg, C) and _ok(dbt, C)
    assert torch.equal(dz[:P * C].cpu(), _bits(dy))


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
def test_zero_z_bn_act_fwd_is_the_rounding_of_beta(with_res):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    P, C = 19, 40
    g = torch.Generator().manual_seed(9)
    beta = torch.rand(C, generator=g) + 0.01                                                # positive fp32, more than 8 bits
    beta[:4] = torch.tensor([0x3f808000, 0x3f818000, 0x3fffffff, 0x3f807fff], dtype=torch.int32).view(torch.float32)
    res = torch.randn(P, C, generator=g).to(torch.bfloat16)
    z = torch.zeros(P, C, dtype=torch.bfloat16, device=DEV)
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    y = _buf16(P * C)
    rd, bd = res.to(DEV), beta.to(DEV)
    _ffi.check(lib.yv3_train_bn_act_fwd_bf16(z.data_ptr(), zero.data_ptr(), one.data_ptr(), one.data_ptr(), bd.data_ptr(),
                                             rd.data_ptr() if with_res else None, y.data_ptr(), P, C, s))
    torch.cuda.synchronize()
    assert _ok(y, P * C)
    want = beta.expand(P, C) + res.float() if with_res else beta.expand(P, C)               # (one fp32 add)
    assert not torch.equal(_bits(beta).view(torch.bfloat16).float(), beta)
    assert torch.equal(y[:P * C].view(P, C).cpu(), _bits(want))


# ---------------------------------------------------------------- values against float64 from the same bf16 / fp32 inputs
def bn_data_b(P, C, seed, ill=False):
    """tests/test_gpu_train_edges.py's inputs with z and res as the kernels take them: bf16 values."""
    d = bn_data(P, C, seed, ill)
    d["z"], d["res"] = K.rb(d["z"]), K.rb(d["res"])
    return d


def gpu_bn_b(d, train):
    """The four bf16 kernels on d -> dict of results (fp32 outputs as GPU tensors, bf16 outputs as float64 CPU values)."""
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    P, C = d["z"].shape
    t = {k_: v.float().contiguous().to(DEV) for k_, v in d.items()}
    zb, rb_ = t["z"].to(torch.bfloat16), t["res"].to(torch.bfloat16)
    assert torch.equal(zb.float(), t["z"]) and torch.equal(rb_.float(), t["res"])
    mean, invstd, rmo, rvo = _buf(C), _buf(C), _buf(C), _buf(C)
    ws, nb = _ws(P, C)
    out = {}
    if train:
        stats = lambda rmi, rvi, o1, o2, m, i, n=nb: lib.yv3_train_bn_stats_bf16(zb.data_ptr(), P, C, K.EPS, K.MOMENTUM, _p(rmi), _p(rvi), _p(o1),
                                                                                 _p(o2), m.data_ptr(), i.data_ptr(), ws.data_ptr(), n, s)
        assert stats(t["rm"], t["rv"], rmo, rvo, mean, invstd, nb - 1) == _ffi.EWORKSPACE
        _ffi.check(stats(t["rm"], t["rv"], rmo, rvo, mean, invstd))
        rma, rva, m2, i2 = _buf(C), _buf(C), _buf(C), _buf(C)                                # run_*_out aliasing run_*
        rma[:C], rva[:C] = t["rm"], t["rv"]
        _ffi.check(stats(rma, rva, rma, rva, m2, i2))
        torch.cuda.synchronize()
        for b_ in (rmo, rvo, rma, rva, m2, i2):
            assert _ok(b_, C)
        assert torch.equal(rma[:C], rmo[:C]) and torch.equal(rva[:C], rvo[:C])
        assert torch.equal(m2[:C], mean[:C]) and torch.equal(i2[:C], invstd[:C])
        out.update(rm=rmo[:C], rv=rvo[:C])
    else:
        _ffi.check(lib.yv3_train_bn_eval_stats(t["rm"].data_ptr(), t["rv"].data_ptr(), K.EPS, mean.data_ptr(), invstd.data_ptr(), C, s))
    y, y0, dz, dgam, dbet = _buf16(P * C), _buf16(P * C), _buf16(P * C), _buf(C), _buf(C)
    for res, dst in ((rb_, y), (None, y0)):
        _ffi.check(lib.yv3_train_bn_act_fwd_bf16(zb.data_ptr(), mean.data_ptr(), invstd.data_ptr(), t["gam"].data_ptr(), t["bet"].data_ptr(),
                                                 _p(res), dst.data_ptr(), P, C, s))
    bwd = lambda n: lib.yv3_train_bn_act_bwd_bf16(zb.data_ptr(), t["dy"].data_ptr(), mean.data_ptr(), invstd.data_ptr(), t["gam"].data_ptr(),
                                                  t["bet"].data_ptr(), dz.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), P, C, train,
                                                  ws.data_ptr(), n, s)
    assert bwd(nb - 1) == _ffi.EWORKSPACE
    _ffi.check(bwd(nb))
    torch.cuda.synchronize()
    for b_, n in ((mean, C), (invstd, C), (y, P * C), (y0, P * C), (dz, P * C), (dgam, C), (dbet, C)):
        assert _ok(b_, n)
    out.update(mean=mean[:C], invstd=invstd[:C], y=_val(y[:P * C]).view(P, C), y0=_val(y0[:P * C]).view(P, C),
               dz=_val(dz[:P * C]).view(P, C), dgamma=dgam[:C], dbeta=dbet[:C])
    return out


def b16_ratio(got, ref, growth=0.0, mask=None):
    """A bf16 output: |got - ref| <= U |ref| + BN_BAR max|ref| (+ growth); `mask`: elements left out (undecided dz)."""
    tol = U * ref.abs() + K.BN_BAR * max(float(ref.abs().max()), 1e-30) + torch.as_tensor(growth, dtype=torch.float64)
    if mask is not None:
        got = torch.where(mask, ref, got)
    return K.ratio(got, ref, tol)


def check_bn_b(d, train, what):
    ref = bn_reference(d, train)
    assert ref["share"] <= K.KINK_SHARE, "undecided share %.3g" % ref["share"]               # (float64, on the CPU)
    got = gpu_bn_b(d, train)
    worst = {k_: K.bn_ratio(got[k_], ref[k_]) for k_ in ("mean", "invstd") + (("rm", "rv") if train else ())}
    worst.update({k_: b16_ratio(got[k_], ref[k_]) for k_ in ("y", "y0")})
    worst["dz"] = b16_ratio(got["dz"], ref["dz"], ref["dz_growth"], ref["und"])
    worst["dgamma"] = K.bn_ratio(got["dgamma"], ref["dgamma"], ref["S"])
    worst["dbeta"] = K.bn_ratio(got["dbeta"], ref["dbeta"], ref["S"])
    print("bn bf16 %s: undecided share %.3g, worst error / bar %s" % (what, ref["share"], {k_: "%.3g" % v for k_, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("C", [8, 96, 1024])
@pytest.mark.parametrize("P", [1, 7, 169, 5408])
def test_bn_bf16_edges(P, C, train):
    check_bn_b(bn_data_b(P, C, 1000 * P + 2 * C + train), train, "P=%d C=%d train=%d" % (P, C, train))


def test_bn_bf16_above_the_grid():
    """More rows than the elementwise kernels' grids cover in one pass (their threads stride on), above 16 777 216 elements."""
    P, C = 176000, 96
    assert P * C > GRID_STRIDE
    check_bn_b(bn_data_b(P, C, 78), 1, "P=%d C=%d train=1 (strided)" % (P, C))


def test_bn_bf16_ill_conditioned():
    """tests/test_gpu_train_edges.py's two hostile inputs as bf16 values: a constant channel (variance exactly 0), and channels of mean
    +-100 over a spread of 0.1 (in bf16: a few elements off 100 by 0.5).  Each fp32 output's bar is BAR_FACTOR times the error of
    torch's fp32 CPU run of the same op; a bf16 output adds its one rounding, U |ref|."""
    P, C = 338, 32
    d = bn_data_b(P, C, 12, ill=True)
    assert float(d["z"][:, 0].std()) == 0.0 and 0.0 < float(d["z"][:, 1].std()) < 0.2
    ref, ref32 = bn_reference(d, 1), bn_reference(d, 1, torch.float32)
    assert ref["share"] == 0.0
    assert float(ref["invstd"][0]) == pytest.approx(1.0 / np.sqrt(K.EPS), rel=1e-12)
    got = gpu_bn_b(d, 1)
    rows_ = []
    for k_ in ("rm", "rv", "y", "y0", "dz", "dgamma", "dbeta"):
        g_ = got[k_].double().cpu()
        assert torch.isfinite(g_).all(), k_
        yard = BAR_FACTOR * float((ref32[k_] - ref[k_]).abs().max())
        tol = yard + (U * ref[k_].abs() if k_ in ("y", "y0", "dz") else 0.0)
        rows_.append((k_, K.ratio(g_, ref[k_], tol + 1e-300)))
    print("bn bf16 ill-conditioned, error / bar (%g x torch fp32 CPU error [+ one bf16 rounding]):" % BAR_FACTOR,
          [(k_, "%.3g" % r) for k_, r in rows_])
    assert torch.isfinite(got["mean"]).all() and torch.isfinite(got["invstd"]).all()
    for k_, r in rows_:
        assert r <= 1.0, (k_, r)
