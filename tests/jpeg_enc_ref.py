"""libjpeg's baseline encoder restated in numpy (plain Python, no GPU): the bytes ``Image.fromarray(a).save(f, "JPEG", quality=q,
subsampling=s)`` writes -- standard Huffman tables, no ``optimize``, no restart markers.  The oracle of the encoder tests is PIL
itself (`jpeg_craft.pil_bytes`); this restatement is what the tests read tokens and scan bits from, and is itself held to PIL's
bytes in tests/test_jpeg_enc_host.py.  The Annex K base tables and the Huffman tables are read from files PIL writes."""
import io
import struct

import numpy as np
from PIL import Image

from jpeg_craft import NATURAL_OF_ZIGZAG, _Bits, _put_block, huffman_codes, segment, standard_tables

SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}      # luma sampling factors (h, v)
PIL_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}

_base = None


def base_tables():
    """The two Annex K tables (natural order), from the DQT segments of a quality-50 file, where their scale is 100 %."""
    global _base
    if _base is None:
        b = io.BytesIO()
        Image.fromarray(np.zeros((8, 8, 3), np.uint8), "RGB").save(b, "JPEG", quality=50)
        data, pos, out = b.getvalue(), 2, {}
        while data[pos + 1] != 0xDA:
            length = struct.unpack(">H", data[pos + 2:pos + 4])[0]
            if data[pos + 1] == 0xDB:
                p, end = pos + 4, pos + 2 + length
                while p < end:
                    assert data[p] >> 4 == 0
                    nat = [0] * 64
                    for k in range(64):
                        nat[NATURAL_OF_ZIGZAG[k]] = data[p + 1 + k]
                    out[data[p] & 15] = nat
                    p += 65
            pos += 2 + length
        assert sorted(out) == [0, 1]
        _base = out
    return _base


def quant_tables(quality):
    """{0: luma, 1: chroma}, 64 values each in natural order (jpeg_set_quality with force_baseline)."""
    assert 1 <= quality <= 100
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return {t: [min(max((v * scale + 50) // 100, 1), 255) for v in base] for t, base in base_tables().items()}


def rgb_to_ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, rows, cols):
    """Repeat the last row and the last column up to rows x cols."""
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode="edge")


def component_plane(full, h, v, blocks_w, blocks_h):
    """The component's samples, blocks_h * 8 rows by blocks_w * 8 columns, from the full-resolution plane ``full``, downsampled by
    h x v: the row is padded to the right at full resolution; at the bottom the last full-resolution row is repeated up to a
    multiple of v, the plane is downsampled, and then the last DOWNSAMPLED row is repeated."""
    H = full.shape[0]
    rows_full = (H + v - 1) // v * v
    p = _pad(full, rows_full, blocks_w * 8 * h).astype(np.int64)
    if (h, v) == (2, 2):
        bias = np.where(np.arange(blocks_w * 8) % 2 == 0, 1, 2)
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias[None, :]) >> 2
    elif (h, v) == (2, 1):
        bias = np.where(np.arange(blocks_w * 8) % 2 == 0, 0, 1)
        p = (p[:, 0::2] + p[:, 1::2] + bias[None, :]) >> 1
    else:
        assert (h, v) == (1, 1)
    return _pad(p, blocks_h * 8, blocks_w * 8)


_F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819,
          f2562=20995, f3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """jfdctint's butterfly along the last axis of ``d`` [..., 8] (int64)."""
    F = _F
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = 13 - 2 if first else 13 + 2
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F["f0541"]
    out[..., 2] = _descale(z1 + t13 * F["f0765"], n)
    out[..., 6] = _descale(z1 - t12 * F["f1847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F["f1175"]
    t4, t5, t6, t7 = t4 * F["f0298"], t5 * F["f2053"], t6 * F["f3072"], t7 * F["f1501"]
    z1, z2, z3, z4 = -z1 * F["f0899"], -z2 * F["f2562"], -z3 * F["f1961"] + z5, -z4 * F["f0390"] + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def fdct_quantise(plane, q):
    """Quantised coefficients ``[rows / 8][cols / 8][64]`` (natural order) of a sample plane: jfdctint on ``sample - 128``, rows
    then columns, then libjpeg's rounding division by ``8 * q``."""
    rows, cols = plane.shape
    b = (plane.astype(np.int64) - 128).reshape(rows // 8, 8, cols // 8, 8).transpose(0, 2, 1, 3)     # [r][c][y][x]
    b = _fdct_pass(b, True)
    b = _fdct_pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)
    c = b.reshape(rows // 8, cols // 8, 64)
    d = 8 * np.asarray(q, np.int64)
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def coefficients(array, quality=75, subsampling="4:2:0"):
    """``(components, (h, v))``: per component ``coef[block rows][block cols][64]`` covering whole MCUs, dummy blocks included
    (all AC 0, DC of the block before them in the MCU's block order).  A 2-D array is a grey image (one component)."""
    a = np.asarray(array)
    assert a.dtype == np.uint8
    q = quant_tables(quality)
    H, W = a.shape[:2]
    if a.ndim == 2:
        bw, bh = (W + 7) // 8, (H + 7) // 8
        return [fdct_quantise(component_plane(a, 1, 1, bw, bh), q[0])], (1, 1)
    h, v = SUBSAMPLING[subsampling]
    mcu_w, mcu_h = (W + 8 * h - 1) // (8 * h), (H + 8 * v - 1) // (8 * v)
    y, cb, cr = rgb_to_ycc(a)
    bw, bh = (W + 7) // 8, (H + 7) // 8                                # real luma blocks
    luma = np.zeros((mcu_h * v, mcu_w * h, 64), np.int64)
    luma[:bh, :bw] = fdct_quantise(component_plane(y, 1, 1, bw, bh), q[0])
    for my in range(mcu_h):
        for mx in range(mcu_w):
            prev = None
            for vy in range(v):
                for hx in range(h):
                    r, c = my * v + vy, mx * h + hx
                    if r >= bh or c >= bw:
                        luma[r, c, 0] = prev
                    prev = luma[r, c, 0]
    cw, ch = ((W + h - 1) // h + 7) // 8, ((H + v - 1) // v + 7) // 8
    assert (cw, ch) == (mcu_w, mcu_h)
    return [luma, fdct_quantise(component_plane(cb, h, v, cw, ch), q[1]), fdct_quantise(component_plane(cr, h, v, cw, ch), q[1])], (h, v)


def header(width, height, ncomp, subsampling="4:2:0", quality=75):
    """Every byte up to and including the SOS segment, in PIL's order: SOI, APP0, one DQT per table, SOF0, DHT DC0 AC0 (DC1 AC1),
    SOS."""
    q, huff = quant_tables(quality), standard_tables()
    h, v = SUBSAMPLING[subsampling] if ncomp == 3 else (1, 1)
    out = bytearray(b"\xff\xd8") + segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2 if ncomp == 3 else 1):
        out += segment(0xDB, bytes([t]) + bytes(q[t][NATURAL_OF_ZIGZAG[k]] for k in range(64)))
    comps = [(1, h << 4 | v, 0), (2, 0x11, 1), (3, 0x11, 1)][:ncomp]
    out += segment(0xC0, struct.pack(">BHHB", 8, height, width, ncomp) + b"".join(bytes(c) for c in comps))
    for t in range(2 if ncomp == 3 else 1):
        for cls in (0, 1):
            counts, values = huff[(cls, t)]
            out += segment(0xC4, bytes([cls << 4 | t]) + bytes(counts) + bytes(values))
    out += segment(0xDA, bytes([ncomp]) + b"".join(bytes([i + 1, 0x11 * min(i, 1)]) for i in range(ncomp)) + b"\x00\x3f\x00")
    return bytes(out)


def scan_blocks(components, hv):
    """``[(component index, coef[64])]`` in scan order: MCU-interleaved for three components, row by row for one."""
    out = []
    if len(components) == 1:
        c = components[0]
        return [(0, c[r, col]) for r in range(c.shape[0]) for col in range(c.shape[1])]
    h, v = hv
    mcu_h, mcu_w = components[1].shape[:2]
    for my in range(mcu_h):
        for mx in range(mcu_w):
            for vy in range(v):
                for hx in range(h):
                    out.append((0, components[0][my * v + vy, mx * h + hx]))
            out.append((1, components[1][my, mx]))
            out.append((2, components[2][my, mx]))
    return out


class _Count:
    """`_Bits`' interface, keeping only the number of bits put."""

    def __init__(self):
        self.bits = 0

    def put(self, code, length):
        self.bits += length


def scan(components, hv):
    """``(bytes of the entropy-coded scan, its length in bits before padding)``."""
    huff = standard_tables()
    codes = [(huffman_codes(*huff[(0, t)]), huffman_codes(*huff[(1, t)])) for t in (0, 1)]
    bits, count, pred = _Bits(), _Count(), [0, 0, 0]
    for ci, block in scan_blocks(components, hv):
        dc, ac = codes[min(ci, 1)]
        _put_block(count, block, pred[ci], dc, ac)
        pred[ci] = _put_block(bits, block, pred[ci], dc, ac)
    bits.pad()
    return bytes(bits.out), count.bits


def zigzag(block):
    return [int(block[NATURAL_OF_ZIGZAG[k]]) for k in range(64)]


def encode(array, quality=75, subsampling="4:2:0"):
    """The file PIL writes for ``array`` (uint8 ``[H][W][3]`` or ``[H][W]``)."""
    a = np.asarray(array)
    comps, hv = coefficients(a, quality, subsampling)
    return header(a.shape[1], a.shape[0], 1 if a.ndim == 2 else 3, subsampling, quality) + scan(comps, hv)[0] + b"\xff\xd9"


def pixels(kind, w, h, grey, seed):
    """The three kinds of test pixels: ``noise``, ``binary`` (0 / 255 noise) and ``smooth``."""
    rng = np.random.RandomState(seed)
    shape = (h, w) if grey else (h, w, 3)
    if kind == "noise":
        return rng.randint(0, 256, shape).astype(np.uint8)
    if kind == "binary":
        return (rng.randint(0, 2, shape) * 255).astype(np.uint8)
    assert kind == "smooth"
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [127.5 + 127.5 * np.sin(xx / (5.0 + 3 * c) + yy / (7.0 - c) + rng.uniform(0, 6)) for c in range(1 if grey else 3)]
    p = np.rint(np.stack(planes, -1)).astype(np.uint8)
    return p[..., 0] if grey else p


MODES = ("grey", "4:4:4", "4:2:2", "4:2:0")


def pil_file(array, quality, mode):
    """PIL's bytes for ``array`` under ``mode`` (one of `MODES`; ``grey`` takes no subsampling argument)."""
    from jpeg_craft import pil_bytes
    if mode == "grey":
        return pil_bytes(array, quality=quality)
    return pil_bytes(array, quality=quality, subsampling=PIL_SUBSAMPLING[mode])
