"""The grid of descriptors behind tests/golden/conv_select_256cu.json: what yv3_conv2d_form / yv3_conv2d_launches answer for every layer of
the network at the batch sizes and options the product and its measurement tools use, on a 256-CU device.

Nothing is launched by the two queries, so the descriptors carry dummy non-null pointers and the walk runs on the host: without a GPU the
library counts 256 compute units, the MI355X's own number.  tools/make_golden_conv_select.py records the table; tests/test_conv_select_host.py
walks the same grid and compares."""
import ctypes

from yolo_v3_amd import _ffi, arch

F32, BF16, F32X3, F32H2 = _ffi.F32, _ffi.BF16, _ffi.F32X3, _ffi.F32H2
SIZES = (416, 608)
BATCHES = (1, 4, 8, 16, 32, 64)
PTR = 0x10000                      # any non-null address: the queries never dereference it
WINO_MIN_CIN = {F32H2: 256, F32: 64}          # engine.WINO_MIN_CIN / WINO_MIN_CIN_F32

# name -> (dtype, options, tune[0..2], variant); variant: None, "nowino" (no Winograd pointers), "strides" (batch-slice plane strides),
# "ws_short" (wino_ws one byte short of the F(2x2) transform's size)
CONFIGS = {
    "f32": (F32, 0, (0, 0, 0), None),
    "f32.two_lanes": (F32, _ffi.OPT_TWO_LANES, (0, 0, 0), None),
    "f32.wino_always": (F32, _ffi.OPT_WINO_ALWAYS, (0, 0, 0), None),
    "f32.wino4_tiles": (F32, _ffi.OPT_WINO4_TILES, (0, 0, 0), None),
    "f32.nowino": (F32, 0, (0, 0, 0), "nowino"),
    "f32.tune0=10": (F32, 0, (10, 0, 0), None),
    "f32.tune0=11": (F32, 0, (11, 0, 0), None),
    "f32.tune0=13": (F32, 0, (13, 0, 0), None),
    "f32.tune0=14": (F32, 0, (14, 0, 0), None),
    "f32.tune1=1": (F32, 0, (0, 1, 0), None),
    "f32.tune1=3": (F32, 0, (0, 3, 0), None),
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
    dtype, options, tune, variant = CONFIGS[cfg]
    sp, H, W, cin_up = layer
    d = _ffi.ConvDesc()
    d.options = options
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
            d.y, d.dec_out, d.dec_stride, d.dec_out_batch_stride = None, PTR, float(size) / ho, 85 * 3 * ho * wo
            for i in range(6):
                d.dec_anchors[i] = float(arch.DEFAULT_ANCHORS[i])
    if dtype == F32H2 and B * (size // 32) ** 2 <= 1536 and not (options & _ffi.OPT_TWO_LANES):      # engine.SK_AUTO_CELLS
        d.workspace, d.workspace_bytes = PTR, lib.yv3_conv_workspace_bytes()
    eligible = sp.k == 3 and sp.stride == 1 and sp.bn and (
        (dtype == F32H2 and sp.cin >= WINO_MIN_CIN[F32H2]) or (dtype == F32 and sp.cin >= WINO_MIN_CIN[F32] and sp.cout % 128 == 0))
    if eligible and variant != "nowino":
        d.w_wino, d.alpha_wino, d.wino_ws, d.wino_ws_bytes = PTR, PTR, PTR, wino_ws_bytes(lib, dtype, B, size)
        if dtype == F32 and sp.cout % 64 == 0 and (sp.cin == 64 or sp.cin % 128 == 0) and cout_pad == sp.cout:
            d.w_wino4 = PTR
        if variant == "ws_short":
            d.wino_ws_bytes = 2 * 16 * B * ((H + 1) // 2) * ((W + 1) // 2) * sp.cin * 2 - 1
    if variant == "strides":
        cx, hx, wx = (cin_up, H // 2, W // 2) if cin_up else (sp.cin, H, W)
        d.x_plane_stride, d.y_plane_stride = 2 * B * hx * wx * cx, 2 * B * ho * wo * sp.cout
        if cin_up:
            d.x2_plane_stride = 2 * B * H * W * (sp.cin - cin_up)
    return d


def grid(lib):
    """Yields (config, size, B, [75 descriptors])."""
    per_size = {size: layers(size) for size in SIZES}
    for cfg in CONFIGS:
        for size in SIZES:
            for B in BATCHES:
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


def _token(form, launches):
    return "%d" % form if form < 0 and launches == form else "%d%d" % (form, launches)


def table(lib):
    """The whole selection table: {"layers": {"config/size/B": "tokens"}, "errors": {"DTYPE/case": "token"}}; a token is the form and
    the launch count as two digits, or the one negative code both queries return."""
    q = lambda d: _token(lib.yv3_conv2d_form(ctypes.byref(d)), lib.yv3_conv2d_launches(ctypes.byref(d)))
    rows = {"%s/%d/%d" % (cfg, size, B): " ".join(q(d) for d in descs) for cfg, size, B, descs in grid(lib)}
    errors = {"%s/%s" % (dname, name): q(d) for dname, name, d in error_descs()}
    return {"cus": 256, "layers": rows, "errors": errors}
