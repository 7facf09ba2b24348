"""A coefficient-level progressive JPEG writer for tests (plain Python + numpy, no GPU), beside `jpeg_craft` for baseline files:
`write` takes the quantised coefficients and ANY script -- a list of `Scan` -- and codes each scan as ITU T.81 annex G and
libjpeg's jcphuff.c do (DC first / refinement, AC first with EOB runs, AC refinement with correction bits).  Every scan gets
Huffman tables of its own, defined right before its SOS: all symbols the scan uses on codes of one length.  `valid_files`,
`crafted`, `refused_scripts` and `damage_sources` are the families the progressive tests share; each is a pure function."""
import collections
import functools
import io
import math
import struct

import numpy as np
from PIL import Image

from tests import jpeg_craft
from tests.jpeg_craft import NATURAL_OF_ZIGZAG, Component, segment

# comps: component indices; restart: the DRI in force (0: none); header_ns: write this many components into the SOS header
# whatever is coded (refused files)
Scan = collections.namedtuple("Scan", "comps ss se ah al restart header_ns", defaults=(0, None))


def pil_script(ncomp):
    """PIL's own script (libjpeg's jpeg_simple_progression)."""
    if ncomp == 1:
        return [Scan((0,), 0, 0, 0, 1), Scan((0,), 1, 5, 0, 2), Scan((0,), 6, 63, 0, 2), Scan((0,), 1, 63, 2, 1), Scan((0,), 0, 0, 1, 0),
                Scan((0,), 1, 63, 1, 0)]
    return [Scan((0, 1, 2), 0, 0, 0, 1), Scan((0,), 1, 5, 0, 2), Scan((2,), 1, 63, 0, 1), Scan((1,), 1, 63, 0, 1), Scan((0,), 6, 63, 0, 2),
            Scan((0,), 1, 63, 2, 1), Scan((0, 1, 2), 0, 0, 1, 0), Scan((2,), 1, 63, 1, 0), Scan((1,), 1, 63, 1, 0), Scan((0,), 1, 63, 1, 0)]


class _Tokens:
    """One unit's symbols and raw bits in order; the codes are assigned when every unit of the scan is known."""

    def __init__(self):
        self.items = []

    def sym(self, table, symbol):
        self.items.append((table, symbol))

    def bits(self, value, n):
        if n:
            self.items.append((None, (value, n)))


def _flat_table(symbols):
    """(counts, values) with every symbol on a code of one length: the shortest that leaves the all-ones code free."""
    values = sorted(symbols) or [0]
    length = max(1, math.ceil(math.log2(len(values) + 1)))
    counts = [0] * 16
    counts[length - 1] = len(values)
    return counts, values


def _blocks(scan, components, width, height):
    """The scan's blocks in coding order: a list of items (MCUs, or the blocks of the one component's own grid), each a list of
    (index into scan.comps, 64 coefficients)."""
    ncomp = len(components)
    hmax, vmax = (1, 1) if ncomp == 1 else (components[0].h, components[0].v)
    if len(scan.comps) > 1:
        mcu_w, mcu_h = -(-width // (8 * hmax)), -(-height // (8 * vmax))
        out = []
        for my in range(mcu_h):
            for mx in range(mcu_w):
                item = []
                for j, c in enumerate(scan.comps):
                    comp = components[c]
                    for vy in range(comp.v):
                        for hx in range(comp.h):
                            item.append((j, comp.coef[my * comp.v + vy, mx * comp.h + hx]))
                out.append(item)
        return out
    comp = components[scan.comps[0]]
    h, v = (1, 1) if ncomp == 1 else (comp.h, comp.v)
    wc, hc = -(-(-(-width * h // hmax)) // 8), -(-(-(-height * v // vmax)) // 8)
    return [[(0, comp.coef[by, bx])] for by in range(hc) for bx in range(wc)]


def _code_unit(scan, items, max_eobrun):
    """The tokens of one unit (jcphuff.c).  Tables are named ("dc", j) per component of the scan and ("ac",)."""
    t = _Tokens()
    al = scan.al
    if scan.ss == 0:
        pred = [0] * len(scan.comps)
        for item in items:
            for j, block in item:
                v = int(block[0]) >> al                               # the point transform of DC is an arithmetic shift
                if scan.ah == 0:
                    diff = v - pred[j]
                    pred[j] = v
                    size = abs(diff).bit_length()
                    t.sym(("dc", j), size)
                    t.bits(diff if diff >= 0 else diff + (1 << size) - 1, size)
                else:
                    t.bits(v & 1, 1)
        return t
    state = {"run": 0, "pending": []}                                 # the EOB run and the correction bits that follow its code

    def flush():
        if state["run"]:
            n = state["run"].bit_length() - 1
            t.sym(("ac",), n << 4)
            t.bits(state["run"] & ((1 << n) - 1), n)
            state["run"] = 0
        for bit in state["pending"]:
            t.bits(bit, 1)
        state["pending"] = []

    for item in items:
        block = item[0][1]
        mag = [abs(int(block[NATURAL_OF_ZIGZAG[k]])) >> al for k in range(64)]     # AC: the shift of the magnitude
        neg = [int(block[NATURAL_OF_ZIGZAG[k]]) < 0 for k in range(64)]
        r = 0
        if scan.ah == 0:
            for k in range(scan.ss, scan.se + 1):
                if mag[k] == 0:
                    r += 1
                    continue
                flush()
                while r > 15:
                    t.sym(("ac",), 0xF0)
                    r -= 16
                size = mag[k].bit_length()
                t.sym(("ac",), r << 4 | size)
                t.bits(mag[k] if not neg[k] else (~mag[k]) & ((1 << size) - 1), size)
                r = 0
            if r:
                state["run"] += 1
                if state["run"] == max_eobrun:
                    flush()
            continue
        last_new = max([k for k in range(scan.ss, scan.se + 1) if mag[k] == 1], default=-1)
        corr = []
        for k in range(scan.ss, scan.se + 1):
            if mag[k] == 0:
                r += 1
                continue
            while r > 15 and k <= last_new:
                flush()
                t.sym(("ac",), 0xF0)
                r -= 16
                for bit in corr:
                    t.bits(bit, 1)
                corr = []
            if mag[k] > 1:                                            # a coefficient with history: its next bit
                corr.append(mag[k] & 1)
                continue
            flush()
            t.sym(("ac",), r << 4 | 1)
            t.bits(0 if neg[k] else 1, 1)
            for bit in corr:
                t.bits(bit, 1)
            corr, r = [], 0
        if r or corr:
            state["run"] += 1
            state["pending"] += corr
            if state["run"] == max_eobrun or len(state["pending"]) > 937:
                flush()
    flush()
    return t


def write(width, height, components, qtables, script, ids=(1, 2, 3), between=None, max_eobrun=0x7FFF):
    """The bytes of a progressive file.  ``components``: one or three `jpeg_craft.Component` (coefficients over whole MCUs);
    ``qtables``: {id: 64 values, natural order}; ``script``: the `Scan` list, written as it is, whether or not it is a
    progression a decoder takes; ``between``: {scan index: bytes placed before that scan's own segments}."""
    ncomp = len(components)
    assert ncomp in (1, 3)
    out = bytearray(b"\xff\xd8") + segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for tid in sorted(qtables):
        q = [int(v) for v in qtables[tid]]
        out += segment(0xDB, bytes([tid]) + bytes(q[NATURAL_OF_ZIGZAG[k]] for k in range(64)))
    out += segment(0xC2, struct.pack(">BHHB", 8, height, width, ncomp)
                   + b"".join(bytes([ids[i], c.h << 4 | c.v, c.tq]) for i, c in enumerate(components)))
    dri = 0
    for index, scan in enumerate(script):
        out += (between or {}).get(index, b"")
        items = _blocks(scan, components, width, height)
        per = scan.restart or len(items)
        units = [_code_unit(scan, items[i:i + per], max_eobrun) for i in range(0, len(items), per)]
        used = collections.defaultdict(set)
        for u in units:
            for table, payload in u.items:
                if table is not None:
                    used[table].add(payload)
        if scan.ss == 0 and scan.ah == 0:
            for j in range(len(scan.comps)):
                used[("dc", j)].add(0)
        codes, selectors = {}, []
        for j, c in enumerate(scan.comps):
            tid = 0 if c == 0 else 1                                  # luma on table 0, both chroma components on table 1
            selectors.append(tid << 4 | tid)
        if scan.ss == 0 and scan.ah == 0:                             # components that share a selector share the table
            by_id = collections.defaultdict(set)
            for j in range(len(scan.comps)):
                by_id[selectors[j] >> 4] |= used[("dc", j)]
            for tid, symbols in sorted(by_id.items()):
                counts, values = _flat_table(symbols)
                out += segment(0xC4, bytes([tid]) + bytes(counts) + bytes(values))
                table = jpeg_craft.huffman_codes(counts, values)
                for j in range(len(scan.comps)):
                    if selectors[j] >> 4 == tid:
                        codes[("dc", j)] = table
        elif scan.ss > 0:
            counts, values = _flat_table(used[("ac",)])
            out += segment(0xC4, bytes([0x10 | selectors[0] & 15]) + bytes(counts) + bytes(values))
            codes[("ac",)] = jpeg_craft.huffman_codes(counts, values)
        if scan.restart != dri:
            out += segment(0xDD, struct.pack(">H", scan.restart))
            dri = scan.restart
        ns = scan.header_ns or len(scan.comps)
        comps = list(scan.comps) + [c for c in range(ncomp) if c not in scan.comps]
        sel = selectors + [0x11] * 3
        out += segment(0xDA, bytes([ns]) + b"".join(bytes([ids[comps[j]], sel[j]]) for j in range(ns))
                       + bytes([scan.ss, scan.se, scan.ah << 4 | scan.al]))
        for n, u in enumerate(units):
            bits = jpeg_craft._Bits()
            for table, payload in u.items:
                if table is None:
                    bits.put(*payload)
                else:
                    bits.put(*codes[table][payload])
            bits.pad()
            out += bits.out
            if n + 1 < len(units):
                out += bytes([0xFF, 0xD0 + n % 8])
    return bytes(out + b"\xff\xd9")


def pil_bytes(array, **kw):
    return jpeg_craft.pil_bytes(array, progressive=True, **kw)


# ---- the families ----------------------------------------------------------------------------------------------------------------
VALID_SIZES = [(1, 1), (7, 9), (8, 8), (17, 13), (33, 19), (40, 24), (96, 80)]


@functools.lru_cache(maxsize=None)
def valid_files():
    """PIL-written progressive files with their baseline twins: [(name, progressive bytes, baseline bytes)].  Grey and the three
    subsamplings, seven sizes, quality 30 / 75 / 95, optimize on and off, no restarts and restart_marker_blocks 1 and 3."""
    out = []
    for mode, sub in (("L", None), ("RGB", 0), ("RGB", 1), ("RGB", 2)):
        for (w, h) in VALID_SIZES:
            a = np.random.RandomState(w * 100 + h).randint(0, 256, (h, w) if mode == "L" else (h, w, 3))
            for quality in (30, 75, 95):
                for optimize in (False, True):
                    for restart in (0, 1, 3):
                        kw = {"quality": quality, "optimize": optimize}
                        if sub is not None:
                            kw["subsampling"] = sub
                        if restart:
                            kw["restart_marker_blocks"] = restart
                        out.append(("pil %s %s %dx%d q%d opt%d rst%d" % (mode, sub, w, h, quality, optimize, restart),
                                    pil_bytes(a, **kw), jpeg_craft.pil_bytes(a, **kw)))
    return out


def _frame(rng, w, h, sampling):
    """Components with ordinary coefficients (`jpeg_craft._ordinary`) and the matching baseline twin's arguments."""
    if sampling is None:
        return [Component(jpeg_craft._ordinary(rng, -(-h // 8), -(-w // 8)))], {0: [4] * 64}
    hs, vs = sampling
    mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
    return ([Component(jpeg_craft._ordinary(rng, mh * vs, mw * hs), hs, vs, 0, 0, 0),
             Component(jpeg_craft._ordinary(rng, mh, mw), 1, 1, 1, 1, 1), Component(jpeg_craft._ordinary(rng, mh, mw), 1, 1, 1, 1, 1)],
            {0: [3] * 64, 1: [5] * 64})


def _twin(w, h, comps, q):
    huff = jpeg_craft._std() if len(comps) == 1 else jpeg_craft._std((0,), (1,), (0,), (1,))
    return jpeg_craft.write(w, h, comps, q, huff)


@functools.lru_cache(maxsize=None)
def crafted(seed=11):
    """Files PIL's encoder never writes: [(name, progressive bytes, baseline twin)]."""
    rng = np.random.RandomState(seed)
    out = []

    def add(name, w, h, comps, q, script, **kw):
        out.append((name, write(w, h, comps, q, script, **kw), _twin(w, h, comps, q)))

    comps, q = _frame(rng, 33, 19, (2, 2))
    add("spectral selection only", 33, 19, comps, q,
        [Scan((0, 1, 2), 0, 0, 0, 0), Scan((0,), 1, 5, 0, 0), Scan((0,), 6, 63, 0, 0), Scan((1,), 1, 63, 0, 0), Scan((2,), 1, 63, 0, 0)])
    comps, q = _frame(rng, 40, 24, None)
    add("al 3, three refinements", 40, 24, comps, q,
        [Scan((0,), 0, 0, 0, 3)] + [Scan((0,), 0, 0, a + 1, a) for a in (2, 1, 0)]
        + [Scan((0,), 1, 9, 0, 3), Scan((0,), 10, 63, 0, 3)] + [Scan((0,), s, e, a + 1, a) for a in (2, 1, 0) for s, e in ((1, 9), (10, 63))])
    comps, q = _frame(rng, 17, 13, (2, 1))
    add("dc one component at a time", 17, 13, comps, q,
        [Scan((c,), 0, 0, 0, 1) for c in (0, 1, 2)] + [Scan((c,), 1, 63, 0, 0) for c in (2, 0, 1)] + [Scan((c,), 0, 0, 1, 0) for c in (1, 2, 0)])
    comps, q = _frame(rng, 33, 19, (2, 2))
    add("dc of two components interleaved", 33, 19, comps, q,
        [Scan((0,), 0, 0, 0, 0), Scan((1, 2), 0, 0, 0, 0)] + [Scan((c,), 1, 63, 0, 0) for c in (0, 1, 2)])
    comps, q = _frame(rng, 24, 16, None)
    add("bands 1-1 and 63-63", 24, 16, comps, q,
        [Scan((0,), 0, 0, 0, 0), Scan((0,), 1, 1, 0, 1), Scan((0,), 63, 63, 0, 0), Scan((0,), 2, 62, 0, 0), Scan((0,), 1, 1, 1, 0)])
    # an EOB run of 16510 blocks (EOB14, the longest code) that spans 128 block rows of a 129-block-wide grid
    c = np.zeros((128, 129, 64), np.int64)
    c[..., 0] = rng.randint(-40, 41, (128, 129))
    c[0, 0, NATURAL_OF_ZIGZAG[5]] = 3
    c[127, 128, NATURAL_OF_ZIGZAG[62]] = -2
    add("eob14 across block rows", 1032, 1024, [Component(c)], {0: [4] * 64},
        [Scan((0,), 0, 0, 0, 0), Scan((0,), 1, 63, 0, 1), Scan((0,), 1, 63, 1, 0)])
    # ZRL inside refinement scans: +-1 coefficients (new at Al = 0) behind runs of 16 to 40 zeros, between coefficients with history
    c = np.zeros((2, 3, 64), np.int64)
    c[..., 0] = rng.randint(-40, 41, (2, 3))
    for r in range(2):
        for col in range(3):
            c[r, col, NATURAL_OF_ZIGZAG[1 + col]] = rng.choice([-5, 4, 6])
            c[r, col, NATURAL_OF_ZIGZAG[21 + 3 * r + col]] = rng.choice([-1, 1])
            c[r, col, NATURAL_OF_ZIGZAG[30]] = rng.choice([-3, 2])
            c[r, col, NATURAL_OF_ZIGZAG[63 - col]] = rng.choice([-1, 1])
    add("zrl in refinement", 24, 16, [Component(c)], {0: [4] * 64},
        [Scan((0,), 0, 0, 0, 0), Scan((0,), 1, 63, 0, 1), Scan((0,), 1, 63, 1, 0)])
    comps, q = _frame(rng, 40, 24, (2, 2))
    add("a restart interval per scan", 40, 24, comps, q,
        [s._replace(restart=r) for s, r in zip(pil_script(3), (2, 0, 1, 5, 3, 7, 1, 0, 2, 4))])
    comps, q = _frame(rng, 160, 120, None)                            # 300 blocks, one per unit: 900 units in the first level
    add("more units than lanes", 160, 120, comps, q,
        [Scan((0,), 0, 0, 0, 0, 1), Scan((0,), 1, 5, 0, 0, 1), Scan((0,), 6, 63, 0, 0, 1)])
    comps, q = _frame(rng, 16, 16, None)
    add("64 scans", 16, 16, comps, q, [Scan((0,), 0, 0, 0, 0)] + [Scan((0,), k, k, 0, 0) for k in range(1, 64)])
    return out


@functools.lru_cache(maxsize=None)
def refused_scripts(seed=12):
    """[(name, bytes, the parser's reason as its name in `_ffi`)]: scripts the parser refuses."""
    rng = np.random.RandomState(seed)
    grey, gq = _frame(rng, 24, 16, None)
    col, cq = _frame(rng, 33, 19, (2, 2))
    dc, ac = Scan((0,), 0, 0, 0, 0), Scan((0,), 1, 63, 0, 0)
    dqt = segment(0xDB, bytes([0]) + bytes([7] * 64))
    return [
        ("a final al of 1", write(24, 16, grey, gq, [Scan((0,), 0, 0, 0, 1), ac]), "JPEGP_SCRIPT"),
        ("a missing band", write(24, 16, grey, gq, [dc, Scan((0,), 1, 5, 0, 0)]), "JPEGP_SCRIPT"),
        ("ac before dc", write(24, 16, grey, gq, [ac, dc]), "JPEGP_SCRIPT"),
        ("ah is not al + 1", write(24, 16, grey, gq, [dc, Scan((0,), 1, 63, 0, 2), Scan((0,), 1, 63, 3, 1), Scan((0,), 1, 63, 1, 0)]),
         "JPEGP_SCAN"),
        ("a repeated first scan", write(24, 16, grey, gq, [dc, dc, ac]), "JPEGP_SCRIPT"),
        ("an interleaved ac scan", write(33, 19, col, cq, [Scan((0, 1, 2), 0, 0, 0, 0), Scan((0,), 1, 63, 0, 0, 0, 3),
                                                           Scan((1,), 1, 63, 0, 0), Scan((2,), 1, 63, 0, 0)]), "JPEGP_SCAN"),
        ("a dqt between scans", write(24, 16, grey, gq, [dc, ac], between={1: dqt}), "JPEGP_DQT"),
        ("65 scans", write(24, 16, grey, gq, [Scan((0,), 0, 0, 0, 1), Scan((0,), 0, 0, 1, 0)] + [Scan((0,), k, k, 0, 0) for k in range(1, 64)]),
         "JPEGP_CAPACITY"),
    ]


@functools.lru_cache(maxsize=None)
def damage_sources():
    """The three progressive files whose bytes the damage tests truncate and corrupt."""
    rs = np.random.RandomState
    return [("420 33x19 q75", pil_bytes(rs(31).randint(0, 256, (19, 33, 3)), quality=75, subsampling=2)),
            ("444 24x16 q95 restarts", pil_bytes(rs(32).randint(0, 256, (16, 24, 3)), quality=95, subsampling=0, restart_marker_blocks=2)),
            ("grey 40x24 q50", pil_bytes(rs(33).randint(0, 256, (24, 40)), quality=50))]


DAMAGE_SEEDS = [5, 9, 7]


def scan_data_range(data):
    """[first, last) of a progressive file's bytes from the first scan's data to its EOI marker (the headers between the scans
    lie inside it)."""
    pos = 2
    while data[pos + 1] != 0xDA:
        pos += 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0]
    assert data[-2:] == b"\xff\xd9"
    return pos + 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0], len(data) - 2


def corruptions(data, count, seed):
    """``count`` seeded copies of ``data`` with one byte of `scan_data_range` replaced by another value."""
    rng = np.random.RandomState(seed)
    first, last = scan_data_range(data)
    out = []
    for _ in range(count):
        v = bytearray(data)
        v[rng.randint(first, last)] ^= rng.randint(1, 256)
        out.append(bytes(v))
    return out


def pil_pixels(data):
    """PIL's RGB pixels of ``data``, or None where PIL raises."""
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.asarray(im.convert("RGB"))
    except Exception:
        return None
