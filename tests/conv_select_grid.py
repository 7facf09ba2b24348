"""The grid of descriptors behind tests/golden/conv_select_256cu.json: what yv3_conv2d_form / yv3_conv2d_launches / yv3_conv2d_kernel answer for
every layer of the network at the batch sizes and options the product and its measurement tools use, on a 256-CU device.

Nothing is launched by the queries, so the descriptors carry dummy non-null pointers and the walk runs on the host: without a GPU the
library counts 256 compute units, the MI355X's own number.  tools/make_golden_conv_select.py records the table; tests/test_conv_select_host.py
walks the same grid and compares."""
import ctypes

from yolo_v3_amd import _ffi, arch
from yolo_v3_amd._ffi import OPT_TILE_SHIFT as TS

F32, BF16, F32X3, F32H2 = _ffi.F32, _ffi.BF16, _ffi.F32X3, _ffi.F32H2
SIZES = (416, 608)
BATCHES = (1, 4, 8, 16, 32, 64)
PTR = 0x10000                      # any non-null address: the queries never dereference it
WINO_MIN_CIN = {F32H2: 256, F32: 64}          # engine.WINO_MIN_CIN / WINO_MIN_CIN_F32

# name -> (dtype, options, tune[0..2], variant); variant: None or several joined by "+": "nowino" (no Winograd pointers), "strides" (batch-slice plane strides),
# "ws_short" (wino_ws one byte short of the F(2x2) transform's size), "sk_ws" / "no_sk_ws" (the stream-K workspace at every batch size / at
# none, instead of engine.SK_AUTO_CELLS' rule), "big_min" (big_tile_min = 64)
CONFIGS = {
    "f32": (F32, 0, (0, 0, 0), None),
    "f32.two_lanes": (F32, _ffi.OPT_TWO_LANES, (0, 0, 0), None),
    "f32.wino_always": (F32, _ffi.OPT_WINO_ALWAYS, (0, 0, 0), None),
    "f32.wino4_tiles": (F32, _ffi.OPT_WINO4_TILES, (0, 0, 0), None),
    "f32.nowino": (F32, 0, (0, 0, 0), "nowino"),
    "f32.tune0=10": (F32, 0, (_ffi.T0_WINO4_NEVER, 0, 0), None),
    "f32.tune0=11": (F32, 0, (_ffi.T0_WINO4_ALWAYS, 0, 0), None),
    "f32.tune0=13": (F32, 0, (_ffi.T0_GEMM_NEVER, 0, 0), None),
    "f32.tune0=14": (F32, 0, (_ffi.T0_GEMM_ALWAYS, 0, 0), None),
    "f32.tune1=1": (F32, 0, (0, _ffi.T1_WINO4_NO_EVEN, 0), None),
    "f32.tune1=3": (F32, 0, (0, _ffi.T1_GEMM_ALL_ROWS, 0), None),
    "f32h2": (F32H2, 0, (0, 0, 0), None),
    "f32h2.two_lanes": (F32H2, _ffi.OPT_TWO_LANES, (0, 0, 0), None),
    "f32h2.wino_always": (F32H2, _ffi.OPT_WINO_ALWAYS, (0, 0, 0), None),
    "f32h2.k3s1": (F32H2, _ffi.OPT_K3S1, (0, 0, 0), None),
    "f32h2.nowino": (F32H2, 0, (0, 0, 0), "nowino"),
    "f32h2.strides": (F32H2, 0, (0, 0, 0), "strides"),
    "f32h2.ws_short": (F32H2, 0, (0, 0, 0), "ws_short"),
    "bf16": (BF16, 0, (0, 0, 0), None),
    "bf16.k3s1": (BF16, _ffi.OPT_K3S1, (0, 0, 0), None),
    "f32x3": (F32X3, 0, (0, 0, 0), None),
}
# ... and the settings that move the remaining rules, each on the dtype it applies to and at one (size, B) where it moves them -- MORE_POINTS
# names the others (the fixture's size is bounded: a row per setting and batch size would not fit)
POINT = {F32: (416, 4), F32H2: (416, 64), BF16: (608, 16)}
MORE_POINTS = {
    # "f32h2" itself has the workspace at 416 up to 8 images and at 608 up to 4 (engine.SK_AUTO_CELLS), and none beyond: those rows are not
    # repeated, nor are 608/8 and 608/32 with it and 608/1 and 608/4 without, whose rows equal recorded ones
    "f32h2.sk_ws": ((416, 16), (416, 32), (416, 64), (608, 16), (608, 64)),
    "f32h2.no_sk_ws": ((416, 1), (416, 4), (416, 8)),
    "f32h2.tile=1": ((416, 4), (416, 64)),                                 # (small batch: the forced 256x128 tile on the stream-K schedule)
    "f32h2.tune1=32.sk_ws": ((416, 16),),                                  # (the 256x128 tile runs stream-K only where the four-wave tile is off)
    "f32.tune1=2": ((608, 64),),                                           # (full rounds of F(4x4) items to drop)
    "f32.tune2=3": ((416, 4), (416, 32)),                                  # (forced parts behind full rounds too)
    "f32h2.tune1=2": ((416, 32), (416, 64)),
}
MORE_POINTS.update({"f32.tune0=%d" % t: ((416, 64),) for t in (2, 6, 7, 8, 9)}, **{"f32.nowino4": ((416, 64),)})
MORE_CONFIGS = {
    # tune[0] / tune[1] / tune[2] of exact fp32: direct tiles, the F(2x2) stage's tile, F(4x4) without full rounds / with forced parts
    "f32.tune0=2": (F32, 0, (_ffi.T0_F32_TILE_64, 0, 0), "nowino"),
    "f32.tune0=6": (F32, 0, (_ffi.T0_F32_TILE_128_W4, 0, 0), "nowino"),
    "f32.tune0=7": (F32, 0, (_ffi.T0_F32_TILE_128_1X1, 0, 0), "nowino"),
    "f32.tune0=8": (F32, 0, (_ffi.T0_WINO2_HALF, 0, 0), "nowino4"),
    "f32.tune0=9": (F32, 0, (_ffi.T0_WINO2_FULL, 0, 0), "nowino4"),
    "f32.nowino4": (F32, 0, (0, 0, 0), "nowino4"),
    "f32.tune1=2": (F32, 0, (0, _ffi.T1_WINO4_NO_FULL, 0), None),
    "f32.tune2=2": (F32, 0, (0, 0, 2), None),
    "f32.tune2=3": (F32, 0, (0, 0, 3), None),
    "f32.tune2=6": (F32, 0, (0, 0, 6), None),
    # fp16 planes: forced tiles, the tune[1] bits, the loop, the even Winograd schedule, the stream-K workspace
    "f32h2.tile=1": (F32H2, _ffi.TILE_256x128_W8 << TS, (0, 0, 0), None),
    "f32h2.tile=2": (F32H2, _ffi.TILE_128x128_W8 << TS, (0, 0, 0), None),
    "f32h2.tile=3": (F32H2, _ffi.TILE_128x128_W4 << TS, (0, 0, 0), None),
    "f32h2.tile=4": (F32H2, _ffi.TILE_128x64 << TS, (0, 0, 0), None),
    "f32h2.tile=12": (F32H2, _ffi.TILE_W4_192x128 << TS, (0, 0, 0), None),
    "f32h2.tune1=1": (F32H2, 0, (0, _ffi.T1P_NO_SHORT_K, 0), None),
    "f32h2.tune1=2": (F32H2, 0, (0, _ffi.T1P_WINO_OTHER_LOOP, 0), None),
    "f32h2.tune1=32": (F32H2, 0, (0, _ffi.T1P_NO_W4, 0), None),
    "f32h2.tune1=64": (F32H2, 0, (0, _ffi.T1P_NO_W4_1X1, 0), None),
    "f32h2.tune1=128": (F32H2, 0, (0, _ffi.T1P_NO_W4_3X3, 0), None),
    "f32h2.two_lanes.tune1=256": (F32H2, _ffi.OPT_TWO_LANES, (0, _ffi.T1P_W4_LANES_3X3, 0), None),
    "f32h2.tune1=32.big_min": (F32H2, 0, (0, _ffi.T1P_NO_W4, 0), "big_min"),
    "f32h2.no_pingpong": (F32H2, _ffi.OPT_NO_PINGPONG, (0, 0, 0), None),
    "f32h2.wino_even": (F32H2, _ffi.OPT_WINO_EVEN | _ffi.OPT_WINO_ALWAYS, (0, 0, 0), None),
    "f32h2.sk_ws": (F32H2, 0, (0, 0, 0), "sk_ws"),
    "f32h2.no_sk_ws": (F32H2, 0, (0, 0, 0), "no_sk_ws"),
    "f32h2.tune1=32.sk_ws": (F32H2, 0, (0, _ffi.T1P_NO_W4, 0), "sk_ws"),
    # one bf16 plane: forced tiles, the tune[1] bits, the four-wave tile's threshold, the loop
    "bf16.tile=1": (BF16, _ffi.TILE_256x128_W8 << TS, (0, 0, 0), None),
    "bf16.tile=5": (BF16, _ffi.TILE_256x128_W4 << TS, (0, 0, 0), None),
    "bf16.tile=6": (BF16, _ffi.TILE_256x256 << TS, (0, 0, 0), None),
    "bf16.tile=7": (BF16, _ffi.TILE_256x128_W4_ROLL << TS, (0, 0, 0), None),
    "bf16.tile=8": (BF16, _ffi.TILE_256x256_ROLL << TS, (0, 0, 0), None),
    "bf16.tile=9": (BF16, _ffi.TILE_256x256_ROLL4 << TS, (0, 0, 0), None),
    "bf16.tile=11": (BF16, _ffi.TILE_192x256_ROLL << TS, (0, 0, 0), None),
    "bf16.tile=13": (BF16, _ffi.TILE_256x256_PP3 << TS, (0, 0, 0), None),
    "bf16.tile=14": (BF16, _ffi.TILE_256x256_PP4 << TS, (0, 0, 0), None),
    "bf16.tile=15": (BF16, _ffi.TILE_192x256_PP3 << TS, (0, 0, 0), None),
    "bf16.tile=16": (BF16, _ffi.TILE_192x256_PP4 << TS, (0, 0, 0), None),
    "bf16.tune1=8": (BF16, 0, (0, _ffi.T1P_BF16_ROUND3, 0), None),
    "bf16.tune1=16": (BF16, 0, (0, _ffi.T1P_BF16_NO_192, 0), None),
    "bf16.tune1=512": (BF16, 0, (0, _ffi.T1P_BF16_ROLL, 0), None),
    "bf16.tune1=1024": (BF16, 0, (0, _ffi.T1P_BF16_PP3, 0), None),
    "bf16.tune2=128": (BF16, 0, (0, 0, 128), None),
    "bf16.big_min": (BF16, 0, (0, 0, 0), "big_min"),
    "bf16.no_pingpong": (BF16, _ffi.OPT_NO_PINGPONG, (0, 0, 0), None),
}
ALL_CONFIGS = dict(CONFIGS, **MORE_CONFIGS)


def layers(size):
    """(spec, input H, input W, cin_up) of the 75 convolutions for a size x size image (engine.Plan's wiring)."""
    specs = arch.conv_specs(80)
    out = []
    for sp, (ho, wo) in zip(specs, arch.conv_output_hw(size, 80)):
        cin_up = {"pre_det2.mlist.0": 256, "pre_det3.mlist.0": 128}.get(sp.name, 0)
        out.append((sp, ho * sp.stride, wo * sp.stride, cin_up))
    return out


def wino_ws_bytes(lib, dtype, B, size):
    """engine.Plan's Winograd scratch: the largest eligible layer of the plan."""
    lo = WINO_MIN_CIN[dtype]
    shapes = ((64, 4), (128, 8), (256, 16), (512, 32))
    need = max(lib.yv3_wino_workspace_bytes(B, size // f, size // f, c) for c, f in shapes if c >= min(lo, 512))
    if dtype == F32:
        need = max(need, max(lib.yv3_wino4_workspace_bytes(B, size // f, size // f, c) for c, f in shapes))
    return need


def make_desc(lib, cfg, size, B, layer):
    """The descriptor engine.make_desc builds for this layer (fused decode on the plane modes' heads), with dummy pointers."""
    dtype, options, tune, variant = ALL_CONFIGS[cfg] if cfg in ALL_CONFIGS else WIDE_HEAD_CONFIGS[cfg]
    variant = (variant or "").split("+")
    sp, H, W, cin_up = layer
    d = _ffi.ConvDesc()
    d.options = options
    d.big_tile_min = 64 if "big_min" in variant else 0
    for i, v in enumerate(tune):
        d.tune[i] = v
    d.x, d.w, d.beta, d.y, d.flags = PTR, PTR, PTR, PTR, PTR
    d.alpha = PTR if sp.bn or dtype == F32H2 else None
    d.x2 = PTR if cin_up else None
    d.residual = PTR if sp.res2 else None
    d.B, d.H, d.W = B, H, W
    cout_pad = (sp.cout + 31) // 32 * 32
    if dtype != F32 and cout_pad > 128:
        cout_pad = (cout_pad + 127) // 128 * 128
    d.cin, d.cin_up, d.cout, d.cout_pad, d.k, d.stride = sp.cin, cin_up, sp.cout, cout_pad, sp.k, sp.stride
    d.act = _ffi.ACT_LEAKY if sp.bn else _ffi.ACT_LINEAR
    d.dtype = d.out_dtype = dtype
    ho, wo = H // sp.stride, W // sp.stride
    if not sp.bn:
        d.out_dtype = F32
        if dtype != F32:                                   # fused decode: the logits are not materialised
            d.y, d.dec_out, d.dec_stride, d.dec_out_batch_stride = None, PTR, float(size) / ho, sp.cout * ho * wo
            for i in range(6):
                d.dec_anchors[i] = float(arch.DEFAULT_ANCHORS[i])
    sk_auto = B * (size // 32) ** 2 <= 1536 and not (options & _ffi.OPT_TWO_LANES)                   # engine.SK_AUTO_CELLS
    if dtype == F32H2 and "no_sk_ws" not in variant and (sk_auto or "sk_ws" in variant):
        d.workspace, d.workspace_bytes = PTR, lib.yv3_conv_workspace_bytes()
    eligible = sp.k == 3 and sp.stride == 1 and sp.bn and (
        (dtype == F32H2 and sp.cin >= WINO_MIN_CIN[F32H2]) or (dtype == F32 and sp.cin >= WINO_MIN_CIN[F32] and sp.cout % 128 == 0))
    if eligible and "nowino" not in variant:
        d.w_wino, d.alpha_wino, d.wino_ws, d.wino_ws_bytes = PTR, PTR, PTR, wino_ws_bytes(lib, dtype, B, size)
        if dtype == F32 and sp.cout % 64 == 0 and (sp.cin == 64 or sp.cin % 128 == 0) and cout_pad == sp.cout and "nowino4" not in variant:
            d.w_wino4 = PTR
        if "ws_short" in variant:
            d.wino_ws_bytes = 2 * 16 * B * ((H + 1) // 2) * ((W + 1) // 2) * sp.cin * 2 - 1
    if "strides" in variant:
        cx, hx, wx = (cin_up, H // 2, W // 2) if cin_up else (sp.cin, H, W)
        d.x_plane_stride, d.y_plane_stride = 2 * B * hx * wx * cx, 2 * B * ho * wo * sp.cout
        if cin_up:
            d.x2_plane_stride = 2 * B * H * W * (sp.cin - cin_up)
    return d


# ----------------------------------------------------------------------------- heads wider than 256 channels (tests/golden/conv_select_wide_heads.json)
F16 = _ffi.F16
WIDE_HEAD_CLASSES = (81, 82, 91, 123, 166, 300)          # cout = 3 * (5 + C) = 258, 261, 288, 384, 513, 915
WIDE_HEAD_BATCHES = (2, 32, 65)                          # 13 x 13 pixels each: M = 338, 5408, and 10985 -- 86 row tiles of 128 x 3 channel tiles of
#                                                          cout 384 = 258 GEMM tiles, the first batch that fills one round of 256 CUs in exact fp32
WIDE_HEAD_CONFIGS = dict({k: CONFIGS[k] for k in ("f32", "f32.tune0=13", "f32.tune0=14", "f32h2", "f32x3", "bf16")}, f16=(F16, 0, (0, 0, 0), None))


def wide_head_desc(lib, cfg, C, B):
    """The descriptor engine.make_desc builds for the 13 x 13 head (cin 256 here, as the kernel tests') of a network with C classes at 416 x 416."""
    sp = arch.ConvSpec("head%d" % C, 256, 3 * (5 + C), 1, 1, False, False)
    return make_desc(lib, cfg, 416, B, (sp, 13, 13, 0))


def wide_heads_table(lib, kernels=()):
    """{"cus", "kernels", "heads": {"config/C/M": token}}: the table's token form (see table()) for every math mode, class count and batch above."""
    kernels = list(kernels)
    heads = {"%s/%d/%d" % (cfg, C, B * 169): _token(query(lib, wide_head_desc(lib, cfg, C, B)), kernels)
             for cfg in WIDE_HEAD_CONFIGS for C in WIDE_HEAD_CLASSES for B in WIDE_HEAD_BATCHES}
    return {"cus": 256, "heads": heads, "kernels": kernels}


def classes(size):
    """(the distinct layers among the 75, [75 indices into them]): the residual blocks repeat their two convolutions, and equal layers get
    equal descriptors, so the table keeps one token per distinct layer and this map."""
    distinct, shapes, index = [], [], []
    for sp, H, W, cin_up in layers(size):
        shape = (sp[1:], H, W, cin_up)                 # make_desc reads nothing else (the name only gave cin_up)
        if shape not in shapes:
            shapes.append(shape)
            distinct.append((sp, H, W, cin_up))
        index.append(shapes.index(shape))
    return distinct, index


def grid(lib):
    """Yields (config, size, B, [one descriptor per distinct layer])."""
    per_size = {size: classes(size)[0] for size in SIZES}
    points = [(cfg, size, B) for cfg in CONFIGS for size in SIZES for B in BATCHES] + [(cfg, size, B) for cfg in MORE_CONFIGS for size, B in MORE_POINTS.get(cfg, (POINT[MORE_CONFIGS[cfg][0]],))]
    for cfg, size, B in points:
        yield cfg, size, B, [make_desc(lib, cfg, size, B, layer) for layer in per_size[size]]


def error_descs():
    """Yields (dtype name, case name, descriptor): every invalid descriptor of tests/test_gpu_conv_matrix.py's error-contract test."""
    from tests.test_gpu_conv_matrix import ERROR_CASES
    for dtype, dname in ((F32, "F32"), (BF16, "BF16"), (F32X3, "F32X3"), (F32H2, "F32H2")):
        ptrs = {"x": PTR, "x2": PTR + 0x100, "w": PTR + 0x200, "beta": PTR + 0x300, "dec": PTR + 0x400,
                "other": F32X3 if dtype == F32H2 else F32H2}
        for name, mutate, code_f32, code_planes in ERROR_CASES:
            if (code_f32 if dtype == F32 else code_planes) is None:
                continue
            d = _ffi.ConvDesc()
            d.x, d.w, d.beta, d.y, d.flags = ptrs["x"], ptrs["w"], ptrs["beta"], PTR + 0x500, PTR + 0x600
            d.B, d.H, d.W, d.cin, d.cout, d.cout_pad, d.k, d.stride = 1, 4, 4, 64, 64, 64, 1, 1
            d.act, d.dtype, d.out_dtype = _ffi.ACT_LEAKY, dtype, dtype
            mutate(d, ptrs)
            yield dname, name, d


def query(lib, d):
    """(form, launches, kernel line) of a descriptor, or the one negative code all three queries return, thrice."""
    buf = ctypes.create_string_buffer(_ffi.KERNEL_LINE_BYTES)
    form, launches = lib.yv3_conv2d_form(ctypes.byref(d)), lib.yv3_conv2d_launches(ctypes.byref(d))
    rc = lib.yv3_conv2d_kernel(ctypes.byref(d), buf, len(buf))
    return (form, launches, buf.value.decode() if rc == 0 else rc)


def answers(lib):
    """{"config/size/B": [(form, launches, kernel line) per distinct layer]}, {"DTYPE/case": (code, code, code)}."""
    rows = {"%s/%d/%d" % (cfg, size, B): [query(lib, d) for d in descs] for cfg, size, B, descs in grid(lib)}
    errors = {"%s/%s" % (dname, name): query(lib, d) for dname, name, d in error_descs()}
    return rows, errors


def _token(answer, kernels):
    form, launches, kernel = answer
    if form < 0:
        assert launches == form and kernel == form, answer
        return "%d" % form
    if kernel not in kernels:
        kernels.append(kernel)
    return "%d%d.%d" % (form, launches, kernels.index(kernel))


def parse(token, kernels):
    """A token of the table back to query()'s answer."""
    if token.startswith("-"):
        return (int(token),) * 3
    return int(token[0]), int(token[1]), kernels[int(token[3:])]


def table(lib, kernels=()):
    """The whole selection table: {"kernels": [lines], "layer_of": {size: [75 indices]}, "layers": {"config/size/B": "tokens"}, "errors":
    {"DTYPE/case": "token"}}.  A row has one token per distinct layer of its size (layer_of maps the 75 convolutions to them); a token is the
    form, the launch count and, after the point, the index of yv3_conv2d_kernel's line in "kernels" -- or the one negative code all three
    queries return.  `kernels`: lines that keep their index (a recorded table's), so that a new line moves no old token."""
    kernels = list(kernels)
    rows, errors = answers(lib)
    out = {"cus": 256, "layer_of": {str(size): " ".join(map(str, classes(size)[1])) for size in SIZES},
           "layers": {key: " ".join(_token(a, kernels) for a in row) for key, row in rows.items()},
           "errors": {key: _token(a, kernels) for key, a in errors.items()}}
    out["kernels"] = kernels
    return out
