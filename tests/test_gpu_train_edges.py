"""Every training entry point of the C-ABI (csrc/train.hip, csrc/train_bf16.hip) at the edges of its tiling, against the same operation
in float64 on the CPU (tests/train_kernel_ref.py).  tests/test_gpu_train.py / test_gpu_train_bf16.py run the net's layers at a 64x64
input with B = 2, where every GEMM M is whole tiles and every wgrad K a multiple of the K step; here are the shapes a real step runs
(13 / 26 / 52 at 416: ragged last M tile, K % 32 != 0, a partial last wgrad chunk), H != W, stride 2 on odd sizes, single tiles and a
single pixel, the arguments nothing else passes (bias, accumulate on the fp32 dgrad, run_*_out aliasing run_*), the entry points nothing
else calls (upcat_bwd, bias_bwd, add) and the grid-stride path of the elementwise kernels (above 16 777 216 elements).

Bars (tests/train_kernel_ref.py): CONV_BAR * sum|a||b| per element for conv products, BN_BAR of the largest reference magnitude for
elementwise / per-channel results, the kink rule for the BN backward.  The two ill-conditioned BatchNorm inputs (a constant channel, a
large mean over a small spread) are held to BAR_FACTOR times the error of torch's fp32 CPU run of the same op, per output.  Every
output buffer carries a canary past its end.  Each test prints its worst error / bar ratio (<= 1 passes)."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_kernel_ref as K
from yolo_v3_amd import _ffi, backprop, F32, BF16

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 64
BAR_FACTOR = 16.0
GRID_STRIDE = 16777216          # grid1 caps the grid at 65536 blocks of 256 threads: above this the elementwise kernels loop


def _buf(n, fill=None):
    b = torch.full((n + CANARY,), float("nan"), device=DEV, dtype=torch.float32)
    if fill is not None:
        b[:n] = fill.reshape(-1).to(DEV)
    return b


def _buf16(n):
    return torch.full((n + CANARY,), 0x1234, device=DEV, dtype=torch.int16)


def _ok(b, n):
    if b.dtype == torch.int16:
        return bool((b[n:] == 0x1234).all())
    return bool(torch.isnan(b[n:]).all())


def _p(t):
    return t.data_ptr() if t is not None else None


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _r8(c):
    return (c + 7) // 8 * 8


# ---------------------------------------------------------------- convolution forward / dgrad / wgrad
#        id                B  H    W    cin   cout  k  st  extras
CONV_CASES = [
    ("416-13x13-3x3",     2, 13,  13,  512,  1024, 3, 1, {}),
    ("416-13x13-1x1",     2, 13,  13,  1024, 512,  1, 1, {}),
    ("416-26x26-b3",      3, 26,  26,  256,  512,  3, 1, {}),
    ("416-52x52-b1",      1, 52,  52,  128,  256,  3, 1, {}),
    ("head-255-bias",     2, 52,  52,  256,  255,  1, 1, dict(bias=True)),
    ("route-768",         2, 26,  26,  768,  256,  1, 1, dict(cin_up=256)),
    ("first-416-nchw",    1, 416, 416, 3,    32,   3, 1, dict(nchw=True)),
    ("down-416-s2",       1, 416, 416, 32,   64,   3, 2, {}),
    ("s2-odd-13x21",      3, 13,  21,  32,   64,   3, 2, {}),
    ("1x1-37x41",         2, 37,  41,  64,   32,   1, 1, {}),
    ("b5-7x9",            5, 7,   9,   32,   64,   3, 1, {}),
    ("tiny-5x3",          1, 5,   3,   64,   128,  3, 1, {}),
    ("tiny-3x5-1x1",      1, 3,   5,   1024, 512,  1, 1, {}),
    ("one-pixel",         1, 1,   1,   64,   32,   1, 1, {}),
    ("fwd4x1-dgrad2x2",   1, 20,  12,  128,  64,   1, 1, {}),
]


def conv_case_data(case, bf):
    """The float64 operands (bf16-rounded values for BF16) and the fp32 tensors they come from."""
    name, B, H, W, cin, cout, k, st, ex = case
    cu = ex.get("cin_up", 0)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) + int(bf))
    x32 = torch.randn(B, cin, H, W, generator=g)
    w32 = torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)
    low = None
    if cu:
        low = torch.randn(B, cu, H // 2, W // 2, generator=g)
        x32[:, :cu] = F.interpolate(low, scale_factor=2, mode="nearest")
    Ho, Wo = (H + 2 * ((k - 1) // 2) - k) // st + 1, (W + 2 * ((k - 1) // 2) - k) // st + 1
    dz32 = torch.randn(B, cout, Ho, Wo, generator=g)
    bias = torch.randn(cout, generator=g) if ex.get("bias") else None
    base = torch.randn(B, cin, H, W, generator=g)
    r = K.rb if bf else (lambda t: t)
    return dict(x32=x32, w32=w32, low=low, dz32=dz32, bias=bias, base=base, Ho=Ho, Wo=Wo,
                x64=r(x32).double(), w64=r(w32).double(), dz64=r(dz32).double())


@pytest.mark.parametrize("math", ["f32", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_edges(case, math):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    name, B, H, W, cin, cout, k, st, ex = case
    bf = math == "bf16"
    cu, nchw = ex.get("cin_up", 0), int(bool(ex.get("nchw")))
    assert not bf or nchw or (cin % 8 == 0 and cu % 8 == 0)
    d = conv_case_data(case, bf)
    x64, w64, dz64, Ho, Wo = d["x64"], d["w64"], d["dz64"], d["Ho"], d["Wo"]
    cp = _r8(cout) if bf else cout
    act = (lambda t: t.to(torch.bfloat16)) if bf else (lambda t: t)

    def dev_in(t):                                                   # an activation as the kernels take it
        return act(t if nchw else _nhwc(t)).contiguous().to(DEV)

    xin = dev_in(d["x32"][:, cu:])
    x2 = dev_in(d["low"]) if cu else None
    wsrc = d["w32"].contiguous().to(DEV)
    nw, nwp = cout * cin * k * k, cp * cin * k * k
    if bf:
        wf, wdd = _buf16(nwp), _buf16(nwp)
        _ffi.check(lib.yv3_train_pack_weight_bf16(wsrc.data_ptr(), wf.data_ptr(), wdd.data_ptr(), cout, cin, k, s))
    else:
        wf, wdd = _buf(nw), _buf(nw)
        _ffi.check(lib.yv3_train_pack_weight(wsrc.data_ptr(), wf.data_ptr(), wdd.data_ptr(), cout, cin, k, s))
    torch.cuda.synchronize()
    assert _ok(wf, nwp) and _ok(wdd, nwp)
    if bf:                                                           # both weight images, the padding channel zero
        wr = d["w32"].to(torch.bfloat16)
        ref_wf = torch.zeros(cp, k * k, cin, dtype=torch.bfloat16)
        ref_wf[:cout] = wr.permute(0, 2, 3, 1).reshape(cout, k * k, cin)
        ref_wd = torch.zeros(cin, k * k, cp, dtype=torch.bfloat16)
        ref_wd[:, :, :cout] = wr.permute(1, 2, 3, 0).reshape(cin, k * k, cout)
        assert torch.equal(wf[:nwp].cpu(), ref_wf.view(torch.int16).reshape(-1))
        assert torch.equal(wdd[:nwp].cpu(), ref_wd.view(torch.int16).reshape(-1))
    m = backprop.MATH[BF16 if bf else F32]
    fwd, dgrad, wgrad, wbytes = (backprop.entry(lib, n) for n in (m.conv_fwd_head, m.conv_dgrad, m.conv_wgrad, m.conv_wgrad_ws))
    worst = {}
    # forward (with the bias and with it NULL where the case has one)
    nz = B * Ho * Wo * cout
    for bias in ([d["bias"], None] if d["bias"] is not None else [None]):
        bd = bias.to(DEV) if bias is not None else None
        z = _buf(nz)
        _ffi.check(fwd(xin.data_ptr(), _p(x2), wf.data_ptr(), _p(bd), z.data_ptr(), B, H, W, cin, cu, cout, k, st, nchw, s))
        torch.cuda.synchronize()
        assert _ok(z, nz)
        ref, sc = K.conv_fwd(x64, w64, st, bias.double() if bias is not None else None)
        worst["fwd" + ("+bias" if bias is not None else "")] = K.conv_ratio(z[:nz].view(B, Ho, Wo, cout), _nhwc(ref), _nhwc(sc))
    # dz as the kernels take it (BF16: coutp channels, the padding zero)
    if bf:
        dzp = torch.zeros(B, Ho, Wo, cp, dtype=torch.bfloat16)
        dzp[..., :cout] = _nhwc(d["dz32"]).to(torch.bfloat16)
        dzd = dzp.to(DEV)
    else:
        dzd = _nhwc(d["dz32"]).to(DEV)
    # dgrad on the full cin, overwriting and accumulating (the first layer has none)
    dcat = None
    if not nchw:
        nx = B * H * W * cin
        ref, sc = K.conv_dgrad(x64.shape, w64, dz64, st)
        for acc in (0, 1):
            base = _nhwc(d["base"])
            dx = _buf(nx, base if acc else None)
            _ffi.check(dgrad(dzd.data_ptr(), wdd.data_ptr(), dx.data_ptr(), B, H, W, cin, cout, k, st, acc, s))
            torch.cuda.synchronize()
            assert _ok(dx, nx)
            r_, s_ = (_nhwc(ref) + base.double(), _nhwc(sc) + base.double().abs()) if acc else (_nhwc(ref), _nhwc(sc))
            worst["dgrad acc=%d" % acc] = K.conv_ratio(dx[:nx].view(B, H, W, cin), r_, s_)
            if not acc:
                dcat = dx[:nx].clone()
    # wgrad with the exact workspace; one byte less is refused before any launch
    nb = wbytes(B, H, W, cin, cout, k, st)
    assert nb > 0
    ws = torch.empty(nb, device=DEV, dtype=torch.uint8)
    dw = _buf(nw)
    assert wgrad(xin.data_ptr(), _p(x2), dzd.data_ptr(), dw.data_ptr(), B, H, W, cin, cu, cout, k, st, nchw, ws.data_ptr(), nb - 1, s) \
        == _ffi.EWORKSPACE
    _ffi.check(wgrad(xin.data_ptr(), _p(x2), dzd.data_ptr(), dw.data_ptr(), B, H, W, cin, cu, cout, k, st, nchw, ws.data_ptr(), nb, s))
    torch.cuda.synchronize()
    assert _ok(dw, nw)
    ref, sc = K.conv_wgrad(x64, w64.shape, dz64, st)
    worst["wgrad"] = K.conv_ratio(dw[:nw].view(cout, cin, k, k), ref, sc)
    # the route conv: its dgrad output split by yv3_train_upcat_bwd, against float64 on that very output
    if cu:
        ct = cin - cu
        nl, nt = B * (H // 2) * (W // 2) * cu, B * H * W * ct
        dlow, dtail = _buf(nl), _buf(nt)
        _ffi.check(lib.yv3_train_upcat_bwd(dcat.data_ptr(), dlow.data_ptr(), dtail.data_ptr(), B, H, W, cu, ct, 0, 0, s))
        torch.cuda.synchronize()
        assert _ok(dlow, nl) and _ok(dtail, nt)
        c64 = dcat.view(B, H, W, cin).permute(0, 3, 1, 2).double().cpu()
        rl, sl, rt = K.upcat_bwd(c64, cu)
        worst["upcat dlow"] = K.ratio(dlow[:nl].view(B, H // 2, W // 2, cu), _nhwc(rl), K.BN_BAR * _nhwc(sl) + 1e-30)
        assert torch.equal(dtail[:nt].view(B, H, W, ct).cpu(), _nhwc(rt).float())
    print("%s %s: worst error / bar %s" % (name, math, {k_: "%.3g" % v for k_, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------- upcat_bwd
@pytest.mark.parametrize("geo", [(2, 10, 6, 128, 256), (1, 26, 26, 256, 512), (2, 26, 26, 128, 256), (3, 10, 6, 8, 24)],
                         ids=lambda g: "x".join(map(str, g)))
def test_upcat_bwd(geo):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    B, H, W, cu, ct = geo
    g = torch.Generator().manual_seed(sum(geo))
    dcat = torch.randn(B, H, W, cu + ct, generator=g)
    bl, bt = torch.randn(B, H // 2, W // 2, cu, generator=g), torch.randn(B, H, W, ct, generator=g)
    rl, sl, rt = K.upcat_bwd(dcat.permute(0, 3, 1, 2).double(), cu)
    rl, sl, rt = _nhwc(rl), _nhwc(sl), _nhwc(rt)
    dc = dcat.to(DEV)
    nl, nt = bl.numel(), bt.numel()
    worst = 0.0
    for want_low, want_tail in ((1, 0), (0, 1), (1, 1)):
        for acc_low in (0, 1):
            for acc_tail in (0, 1):
                dlow, dtail = _buf(nl, bl), _buf(nt, bt)                # both pre-filled: an ignored acc flag shows as base + value
                _ffi.check(lib.yv3_train_upcat_bwd(dc.data_ptr(), dlow.data_ptr() if want_low else None,
                                                   dtail.data_ptr() if want_tail else None, B, H, W, cu, ct, acc_low, acc_tail, s))
                torch.cuda.synchronize()
                assert _ok(dlow, nl) and _ok(dtail, nt)
                gl, gt = dlow[:nl].view_as(bl).cpu(), dtail[:nt].view_as(bt).cpu()
                if want_low:
                    ref = rl + bl.double() if acc_low else rl
                    sc = sl + bl.double().abs() if acc_low else sl
                    worst = max(worst, K.ratio(gl, ref, K.BN_BAR * sc + 1e-30))
                else:
                    assert torch.equal(gl, bl)                          # a NULL destination's neighbour is left alone
                if want_tail:                                           # a copy, or one fp32 add: exact
                    assert torch.equal(gt, (bt.double() + rt).float() if acc_tail else rt.float())
                else:
                    assert torch.equal(gt, bt)
    print("upcat_bwd %s: worst error / bar %.3g" % (geo, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------- bias_bwd
@pytest.mark.parametrize("P", [1, 338, 2 * 52 * 52])
@pytest.mark.parametrize("C", [18, 255])
@pytest.mark.parametrize("scale", [None, 0.5, -1.75], ids=["noscale", "half", "negative"])
def test_bias_bwd(scale, C, P):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    g = torch.Generator().manual_seed(P * 3 + C)
    dl = torch.randn(P, C, generator=g)
    sd_ = torch.tensor(scale, dtype=torch.float32, device=DEV) if scale is not None else None
    dout, db = _buf(P * C), _buf(C)
    nb = lib.yv3_train_channel_workspace_bytes(P, C)
    assert nb > 0
    ws = torch.empty(nb, device=DEV, dtype=torch.uint8)
    dld = dl.to(DEV)
    assert lib.yv3_train_bias_bwd(dld.data_ptr(), _p(sd_), dout.data_ptr(), db.data_ptr(), P, C, ws.data_ptr(), nb - 1, s) == _ffi.EWORKSPACE
    _ffi.check(lib.yv3_train_bias_bwd(dld.data_ptr(), _p(sd_), dout.data_ptr(), db.data_ptr(), P, C, ws.data_ptr(), nb, s))
    torch.cuda.synchronize()
    assert _ok(dout, P * C) and _ok(db, C)
    rd, rb_, ra = K.bias_bwd(dl.double(), scale)
    assert torch.equal(dout[:P * C].view(P, C).cpu(), rd.float())       # one fp32 multiply: float64's product rounded once
    worst = K.ratio(db[:C], rb_, K.BN_BAR * ra + 1e-30)
    print("bias_bwd P=%d C=%d scale=%s: worst error / bar %.3g" % (P, C, scale, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------- add, cast: small sizes and the grid-stride loop
@pytest.mark.parametrize("n", [1, 255, GRID_STRIDE + 193])
def test_add_is_exact(n):
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    g = torch.Generator(device=DEV).manual_seed(n % 1000)
    src = torch.randn(n, device=DEV, generator=g)
    base = torch.randn(n, device=DEV, generator=g)
    dst = _buf(n, base)
    _ffi.check(lib.yv3_train_add(src.data_ptr(), dst.data_ptr(), n, s))
    torch.cuda.synchronize()
    assert _ok(dst, n)
    want = (base.double() + src.double()).float()                       # one fp32 add = the float64 sum rounded once
    assert torch.equal(dst[:n], want)


def test_cast_grid_stride_with_padding():
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    C, ld = 255, 256
    rows = GRID_STRIDE // ld + 5
    assert rows * ld > GRID_STRIDE
    a = torch.randn(rows, C, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)) * 7
    d = _buf16(rows * ld)
    _ffi.check(lib.yv3_train_to_bf16(a.data_ptr(), d.data_ptr(), rows, C, ld, s))
    torch.cuda.synchronize()
    assert _ok(d, rows * ld)
    dd = d[:rows * ld].view(rows, ld)
    assert torch.equal(dd[:, :C], a.to(torch.bfloat16).view(torch.int16)) and bool((dd[:, C:] == 0).all())


# ---------------------------------------------------------------- BatchNorm statistics, BN + LeakyReLU forward and backward
def bn_data(P, C, seed, ill=False):
    """fp32-representable float64 inputs of the existing test's distribution; ill: channel 0 constant, channels 1 / 2 a mean of
    +-100 over a spread of 0.1 (their beta keeps u three gammas from 0, so that no fp32 rounding of the mean decides a sign)."""
    g = torch.Generator().manual_seed(seed)
    f = lambda t: t.float().double()
    d = dict(z=f(torch.randn(P, C, generator=g, dtype=torch.float64) * 3 + 1), res=f(torch.randn(P, C, generator=g, dtype=torch.float64)),
             dy=f(torch.randn(P, C, generator=g, dtype=torch.float64)), gam=f(torch.rand(C, generator=g, dtype=torch.float64) + 0.5),
             bet=f(torch.rand(C, generator=g, dtype=torch.float64) - 0.5), rm=f(torch.randn(C, generator=g, dtype=torch.float64)),
             rv=f(torch.rand(C, generator=g, dtype=torch.float64) * 4 + 0.1))
    if ill:
        d["z"][:, 0] = 2.5
        d["bet"][0] = 0.3
        d["z"][:, 1] = f(100 + 0.1 * torch.randn(P, generator=g, dtype=torch.float64))
        d["z"][:, 2] = f(-100 + 0.1 * torch.randn(P, generator=g, dtype=torch.float64))
        d["gam"][1:3] = 0.5
        d["bet"][1], d["bet"][2] = 3.0, -3.0
    return d


def bn_reference(d, train, dtype=torch.float64):
    """mean, invstd, the running statistics, y (with and without the residual) and the backward, in `dtype`.  float64: the closed
    forms of tests/train_kernel_ref.py (checked against autograd here whenever torch has a reference, i.e. P > 1 or eval); float32:
    torch's own F.batch_norm + F.leaky_relu under autograd, the yardstick of the ill-conditioned cases."""
    P = d["z"].shape[0]
    out = {}
    if train and P == 1:
        with pytest.raises(ValueError):                                 # torch refuses one value per channel in training
            F.batch_norm(d["z"].t().unsqueeze(0), d["rm"].clone(), d["rv"].clone(), d["gam"], d["bet"], training=True)
    else:
        zz = d["z"].to(dtype).clone().requires_grad_(True)
        ga, be = d["gam"].to(dtype).clone().requires_grad_(True), d["bet"].to(dtype).clone().requires_grad_(True)
        rm2, rv2 = d["rm"].to(dtype).clone(), d["rv"].to(dtype).clone()
        u = F.batch_norm(zz.t().unsqueeze(0), rm2, rv2, ga, be, training=bool(train), momentum=K.MOMENTUM, eps=K.EPS)
        y0 = F.leaky_relu(u, K.SLOPE)[0].t()
        y0.backward(d["dy"].to(dtype))
        out = dict(y0=y0.detach().double(), y=(y0.detach() + d["res"].to(dtype)).double(), dz=zz.grad.double(), dgamma=ga.grad.double(),
                   dbeta=be.grad.double(), rm=rm2.double(), rv=rv2.double())
        if dtype != torch.float64:
            return out
    if train:
        mean, var, invstd = K.bn_batch_stats(d["z"])
        rm, rv = K.bn_running(mean, var, P, d["rm"], d["rv"])
    else:
        (mean, invstd), rm, rv = K.bn_eval_stats(d["rm"], d["rv"]), d["rm"], d["rv"]
    b = K.bn_act_bwd(d["z"], d["dy"], mean, invstd, d["gam"], d["bet"], train)
    cf = dict(mean=mean, invstd=invstd, rm=rm, rv=rv, y0=K.bn_act_fwd(d["z"], mean, invstd, d["gam"], d["bet"]),
              y=K.bn_act_fwd(d["z"], mean, invstd, d["gam"], d["bet"], d["res"]), **b)
    for k_, v in out.items():                                           # the closed forms are autograd's, to float64 round-off
        assert float((cf[k_] - v).abs().max()) <= 1e-9 * max(float(v.abs().max()), 1e-30), k_
    return cf


def gpu_bn(d, train):
    """The four kernels on d -> dict of the results (GPU tensors), after the canary and aliasing checks."""
    lib, s = _ffi.lib(), _ffi.stream_ptr()
    P, C = d["z"].shape
    t = {k_: v.float().contiguous().to(DEV) for k_, v in d.items()}
    mean, invstd, rmo, rvo = _buf(C), _buf(C), _buf(C), _buf(C)
    nb = lib.yv3_train_channel_workspace_bytes(P, C)
    assert nb > 0
    ws = torch.empty(nb, device=DEV, dtype=torch.uint8)
    out = {}
    if train:
        stats = lambda rmi, rvi, o1, o2, m, i: lib.yv3_train_bn_stats(t["z"].data_ptr(), P, C, K.EPS, K.MOMENTUM, _p(rmi), _p(rvi), _p(o1),
                                                                      _p(o2), m.data_ptr(), i.data_ptr(), ws.data_ptr(), nb, s)
        _ffi.check(stats(t["rm"], t["rv"], rmo, rvo, mean, invstd))
        # run_*_out aliasing run_* (include/yv3.h promises it), and NULL: the same values, nothing else touched
        rma, rva, m2, i2 = _buf(C, t["rm"]), _buf(C, t["rv"]), _buf(C), _buf(C)
        _ffi.check(stats(rma, rva, rma, rva, m2, i2))
        m3, i3 = _buf(C), _buf(C)
        _ffi.check(stats(t["rm"], t["rv"], None, None, m3, i3))
        torch.cuda.synchronize()
        for b_ in (rmo, rvo, rma, rva, m2, i2, m3, i3):
            assert _ok(b_, C)
        assert torch.equal(rma[:C], rmo[:C]) and torch.equal(rva[:C], rvo[:C])
        assert torch.equal(m2[:C], mean[:C]) and torch.equal(i2[:C], invstd[:C])
        assert torch.equal(m3[:C], mean[:C]) and torch.equal(i3[:C], invstd[:C])
        assert torch.equal(t["rm"].cpu(), d["rm"].float()) and torch.equal(t["rv"].cpu(), d["rv"].float())
        out.update(rm=rmo[:C], rv=rvo[:C])
    else:
        _ffi.check(lib.yv3_train_bn_eval_stats(t["rm"].data_ptr(), t["rv"].data_ptr(), K.EPS, mean.data_ptr(), invstd.data_ptr(), C, s))
    y, y0, dz, dgam, dbet = _buf(P * C), _buf(P * C), _buf(P * C), _buf(C), _buf(C)
    for res, dst in ((t["res"], y), (None, y0)):
        _ffi.check(lib.yv3_train_bn_act_fwd(t["z"].data_ptr(), mean.data_ptr(), invstd.data_ptr(), t["gam"].data_ptr(), t["bet"].data_ptr(),
                                            _p(res), dst.data_ptr(), P, C, s))
    _ffi.check(lib.yv3_train_bn_act_bwd(t["z"].data_ptr(), t["dy"].data_ptr(), mean.data_ptr(), invstd.data_ptr(), t["gam"].data_ptr(),
                                        t["bet"].data_ptr(), dz.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), P, C, train,
                                        ws.data_ptr(), nb, s))
    torch.cuda.synchronize()
    for b_, n in ((mean, C), (invstd, C), (y, P * C), (y0, P * C), (dz, P * C), (dgam, C), (dbet, C)):
        assert _ok(b_, n)
    out.update(mean=mean[:C], invstd=invstd[:C], y=y[:P * C].view(P, C), y0=y0[:P * C].view(P, C), dz=dz[:P * C].view(P, C),
               dgamma=dgam[:C], dbeta=dbet[:C])
    return out


def check_bn(d, train, what):
    ref = bn_reference(d, train)
    assert ref["share"] <= K.KINK_SHARE, "undecided share %.3g" % ref["share"]
    got = gpu_bn(d, train)
    worst = {k_: K.bn_ratio(got[k_], ref[k_]) for k_ in ("mean", "invstd", "y", "y0") + (("rm", "rv") if train else ())}
    if not train:
        assert torch.equal(got["mean"].cpu(), d["rm"].float())
    worst.update(K.bn_bwd_ratios(got["dz"], got["dgamma"], got["dbeta"], ref))
    print("bn %s: undecided share %.3g, worst error / bar %s" % (what, ref["share"], {k_: "%.3g" % v for k_, v in worst.items()}))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
@pytest.mark.parametrize("C", [32, 96, 1024])
@pytest.mark.parametrize("P", [1, 3, 64, 65, 338, 2 * 52 * 52])
def test_bn_edges(P, C, train):
    check_bn(bn_data(P, C, 1000 * P + 2 * C + train), train, "P=%d C=%d train=%d" % (P, C, train))


@pytest.mark.parametrize("train", [1, 0], ids=["train", "eval"])
def test_bn_grid_stride(train):
    P, C = 262147, 64
    assert P * C > GRID_STRIDE
    check_bn(bn_data(P, C, 77 + train), train, "P=%d C=%d train=%d (grid-stride)" % (P, C, train))


ILL_SEED = 12


def test_bn_ill_conditioned():
    """A constant channel (variance exactly 0: invstd = 1/sqrt(eps)) and two channels of mean +-100 over a spread of 0.1.  The fp32
    rounding of the mean alone moves xhat by more than BN_BAR there, so each output's bar is BAR_FACTOR times the error torch's fp32
    CPU run of the same op leaves against float64 (max error over max magnitude, the metric of the other cases)."""
    P, C = 338, 32
    d = bn_data(P, C, ILL_SEED, ill=True)
    ref, ref32 = bn_reference(d, 1), bn_reference(d, 1, torch.float32)
    assert ref["share"] == 0.0                                          # (the seed: no element of the reference sits on the kink)
    assert float(ref["invstd"][0]) == pytest.approx(1.0 / np.sqrt(K.EPS), rel=1e-12)
    got = gpu_bn(d, 1)

    def rel(a, k_):
        return float((a.double().cpu() - ref[k_]).abs().max()) / float(ref[k_].abs().max())

    rows_ = []
    for k_, k32 in (("rm", "rm"), ("rv", "rv"), ("y", "y"), ("y0", "y0"), ("dz", "dz"), ("dgamma", "dgamma"), ("dbeta", "dbeta")):
        assert torch.isfinite(got[k_]).all(), k_
        rows_.append((k_, rel(got[k_], k_), BAR_FACTOR * rel(ref32[k32], k_)))
    print("bn ill-conditioned (output, GPU error, bar = %g x torch fp32 CPU error):" % BAR_FACTOR,
          [(k_, "%.3g" % e, "%.3g" % b_) for k_, e, b_ in rows_])
    assert torch.isfinite(got["mean"]).all() and torch.isfinite(got["invstd"]).all()
    for k_, e, b_ in rows_:
        assert e <= b_, (k_, e, b_)
