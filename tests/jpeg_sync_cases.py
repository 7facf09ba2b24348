"""Input files for the workgroup logic of the self-synchronising entropy stage (``entropy_kernel<1>`` and ``sync_unit`` in
csrc/jpeg.hip), which only a GPU run sees: plain Python + numpy + PIL, no GPU, and no libyv3 for anything but ``cuts()`` (whose
files ``test_jpeg_sync_host.find_boundary_files`` finds with the parser).  Every generator is a pure function of its seeds and
returns ``[(name, bytes)]``.  ``EXPECT[name]`` says what each file is meant to be: ``tests/test_jpeg_sync_host.py`` asserts it
with the host program on the CPU, so a generator that stops producing its property fails there, by name, and
``tests/test_gpu_jpeg_sync.py`` gives the same files to the kernel.

The path of the workgroup logic each file reaches (S = 64 bytes a subsequence, 256 lanes a window, 256 units a round):

  a second round of units that holds long units        rounds(): "grey 300 long units" (44 in round two), "4:2:0 512 long units"
  s_long filled to exactly 256 in one round             rounds(): "4:2:0 512 long units", in both rounds
  more long units than lanes                            rounds(): "grey 300 long units", "4:2:0 512 long units"
  a round whose only long units come late               rounds(): "300 segments, long at 260 and 299" (round one: none; round two:
                                                        unit 260 and the image's last unit)
  short and long units interleaved, bpm 6, m0 > 0       rounds(): "4:2:0 stripes"
  nsub = 255: the window's last lane stays empty        window_edges(): "grey noise nsub 255"
  nsub = 256: an exactly full window                    window_edges(): "grey noise nsub 256", "crafted scan of LANES*S bytes"
  nsub = 257: a second window of one lane               window_edges(): "grey noise nsub 257", "crafted scan of LANES*S+1 bytes" (a
                                                        subsequence of one byte)
  a partial commit: a window that ends at np < nl       window_edges(): "noise q100 4:4:4" (windows > ceil(nsub / 256)), and, as
                                                        the host program shows, whichever of the files above needs it
  a stuffing pair cut in two                            cuts(): "00 of a pair first"
  an FF as the first byte of a subsequence              cuts(): "FF first"
  a pair that ends at the cut                           cuts(): "pair ends at the cut"
  scans of S-1 / S / S+1 bytes (one lane, serial)       cuts(): "scan of 63 / 64 / 65 bytes"
  scans of 4S-1 / 4S / 4S+1 and a multiple of S         cuts(): "scan of 255 / 256 / 257 bytes", "scan of multiple bytes" (the
                                                        threshold between one lane and the workgroup; a last subsequence that
                                                        is full, and one of a single byte)
  the DC pass with M < 256 (chunk 1, an empty lane)     dc_shapes(): "4:4:4 255 MCUs"; the striped file's units (20 MCUs)
  the DC pass with M = 256 (chunk 1, every lane)        dc_shapes(): "4:4:4 256 MCUs"
  the DC pass with M = 256 k + 1 (chunk k + 1)          dc_shapes(): "4:4:4 257 MCUs" (lane 128 has one MCU, 127 lanes none),
                                                        "4:4:4 513 MCUs" (chunk 3, 171 lanes)
  handed_over == NULL with the parallel stage           test_gpu_jpeg_sync.test_null_handed_over, over rounds()
  a handed-over unit (zeroed again, decoded serially)   test_gpu_jpeg_sync's damage tests: corruptions of the 512-unit and the
                                                        striped file, and a bit flipped in unit 270 of the 300-unit file
"""
import functools

import numpy as np

from tests import jpeg_craft
from tests.test_jpeg_host import encode, picture
from tests.test_jpeg_sync_host import LANES, MIN_FACTOR, S, find_boundary_files, segments_300, table_files

ROUND = 256                                                       # units a round of entropy_kernel<1>: one lane each

# name -> what the file is meant to be, for the host program's summary at S.  units, long_units, scan_bytes, mcus (of the single
# unit): fixed by the name.  windows: "1", ">=2" or ">ceil" (more windows than ceil(nsub / LANES): a partial commit).
# per_round_meant / long_at_meant: long units in each round of ROUND units / their indices, against per_round / long_at, which
# `unit_lengths` counts in the file as it came out.  nsub: subsequences summed over the long units, fixed by the name where the
# name has it, counted by `unit_lengths` otherwise (a count the host program did not make).
EXPECT = {}


def scan_bytes(data):
    first, last = jpeg_craft.scan_range(data)
    return last - first


def unit_lengths(data):
    """Byte counts of the restart segments of ``data``'s scan."""
    first, last = jpeg_craft.scan_range(data)
    sc, out, begin = data[first:last], [], 0
    for i in range(len(sc) - 1):
        if sc[i] == 0xFF and 0xD0 <= sc[i + 1] <= 0xD7:
            out.append(i - begin)
            begin = i + 2
    return out + [len(sc) - begin]


def nsub_of(lengths):
    return sum(-(-n // S) for n in lengths if n >= MIN_FACTOR * S)


def _expect(name, data, **kw):
    lengths = unit_lengths(data)
    long_at = [u for u, n in enumerate(lengths) if n >= MIN_FACTOR * S]
    kw.setdefault("nsub", nsub_of(lengths))
    kw["per_round"] = tuple(sum(r * ROUND <= u < (r + 1) * ROUND for u in long_at) for r in range(-(-len(lengths) // ROUND)))
    kw["long_at"] = tuple(long_at)
    EXPECT[name] = kw
    return name, data


@functools.lru_cache(maxsize=None)
def rounds():
    out = []
    data = encode(picture(8, 9600, "L", seed=0), quality=100, restart_marker_blocks=4)
    out.append(_expect("grey 300 long units", data, units=300, long_units=300, per_round_meant=(256, 44)))
    data = encode(picture(16, 8192, seed=0), quality=95, subsampling=2, restart_marker_rows=1)
    out.append(_expect("4:2:0 512 long units", data, units=512, long_units=512, per_round_meant=(256, 256)))
    _, data = segments_300(np.random.RandomState(31), (260, 299))
    out.append(_expect("300 segments, long at 260 and 299", data, units=300, long_units=2, per_round_meant=(0, 2),
                       long_at_meant=(260, 299)))
    a = np.asarray(picture(320, 96, seed=0)).copy()
    for row in range(0, 96, 32):
        a[row:row + 16] = 77                                      # MCU rows 0, 2, 4 flat, 1, 3, 5 noise
    data = jpeg_craft.pil_bytes(a, quality=90, subsampling=2, restart_marker_rows=1)
    out.append(_expect("4:2:0 stripes", data, units=6, long_units=3, per_round_meant=(3,), long_at_meant=(1, 3, 5)))
    return out


def _tuned(target, seed):
    """A grey `jpeg_craft` file whose scan has exactly ``target`` bytes: ``n`` ordinary blocks (n by bisection: the longest scan
    below the target), then flat blocks, of which the first ``m`` carry one AC coefficient of 1.  Such a block adds three bits and
    no FF byte, so some m gives every length from there on."""
    rows, cols = 36, 40
    noisy = jpeg_craft._ordinary(np.random.RandomState(seed), 1, rows * cols)[0]

    def build(n, m):
        c = np.zeros((rows * cols, 64), np.int64)
        c[:n] = noisy[:n]
        c[n:n + m, jpeg_craft.NATURAL_OF_ZIGZAG[1]] = 1
        return jpeg_craft._grey("", 8 * cols, 8 * rows, c.reshape(rows, cols, 64))[1]

    def bisect(f, lo, hi):                                        # the largest x in [lo, hi] with f(x) < target (f rising)
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if f(mid) < target else (lo, mid - 1)
        return lo
    spare = 128                                                   # flat blocks kept for m: 48 bytes' worth
    assert scan_bytes(build(0, 0)) < target <= scan_bytes(build(rows * cols - spare, 0)), "the ordinary blocks do not reach the target"
    n = bisect(lambda x: scan_bytes(build(x, 0)), 0, rows * cols - spare)
    m = bisect(lambda x: scan_bytes(build(n, x)), 0, spare) + 1
    for m in range(m, m + 3):                                     # the two or three m of this length: the one whose last symbol, the
        data = build(n, m)                                        # EOB 1010 before the padding ones, begins in the scan's last byte
        assert scan_bytes(data) == target, "no scan of exactly %d bytes: %d" % (target, scan_bytes(data))
        last = data[-3]
        if any(last & ((1 << (pad + 4)) - 1) == (0b1010 << pad | ((1 << pad) - 1)) for pad in range(5)):
            return data
    raise AssertionError("no scan of %d bytes whose last symbol begins in its last byte" % target)


@functools.lru_cache(maxsize=None)
def window_edges():
    """(The search is over seeds 0 to 399 at qualities 74 to 78, seed first; it stops at the first file of each kind.)"""
    want = {LANES - 1: None, LANES: None, LANES + 1: None}
    for seed in range(400):
        im = picture(280, 104, "L", seed=seed)
        for quality in range(74, 79):
            data = encode(im, quality=quality)
            nsub = -(-scan_bytes(data) // S)
            if nsub in want and want[nsub] is None:
                want[nsub] = data
        if all(v is not None for v in want.values()):
            break
    missing = [k for k, v in want.items() if v is None]
    assert not missing, "the search found no grey 280x104 noise file of %s subsequences" % missing
    out = [_expect("grey noise nsub %d" % k, want[k], units=1, long_units=1, nsub=k, windows="1" if k <= LANES else ">=2")
           for k in sorted(want)]
    out.append(_expect("crafted scan of LANES*S bytes", _tuned(LANES * S, 41), units=1, long_units=1, nsub=LANES, windows="1",
                       scan_bytes=LANES * S))
    out.append(_expect("crafted scan of LANES*S+1 bytes", _tuned(LANES * S + 1, 42), units=1, long_units=1, nsub=LANES + 1, windows=">=2",
                       scan_bytes=LANES * S + 1))
    name, data = table_files()[4]
    assert name == "noise q100 4:4:4"
    out.append(_expect(name, data, units=1, long_units=1, windows=">ceil"))
    return out


@functools.lru_cache(maxsize=None)
def cuts():
    found, want, lengths, targets = find_boundary_files()
    assert set(found) == set(want) and set(lengths) == set(targets), "find_boundary_files no longer finds every file"
    out = [_expect(name, found[name], units=1, long_units=1) for name in want]
    for n in targets:
        data = lengths[n]
        long = n == "multiple" or n >= MIN_FACTOR * S
        out.append(_expect("scan of %s bytes" % n, data, units=1, long_units=int(long), **({} if n == "multiple" else {"scan_bytes": n})))
    return out


@functools.lru_cache(maxsize=None)
def dc_shapes():
    out = []
    for mcus in (LANES - 1, LANES, LANES + 1, 2 * LANES + 1):
        data = encode(picture(8 * mcus, 8, seed=mcus), quality=75, subsampling=0)
        out.append(_expect("4:4:4 %d MCUs" % mcus, data, units=1, long_units=1, mcus=mcus))
    return out


def damaged_round_two():
    """"grey 300 long units" with one bit flipped in the middle of unit 270, a long unit of the second round."""
    data = bytearray(dict(rounds())["grey 300 long units"])
    lengths = unit_lengths(data)
    at = jpeg_craft.scan_range(data)[0] + sum(n + 2 for n in lengths[:270]) + lengths[270] // 2
    assert data[at] not in (0, 0xFF) and (data[at] ^ 0x10) not in (0, 0xFF)       # the flip makes and breaks no marker or stuffing pair
    data[at] ^= 0x10
    return "grey 300 long units, a bit flipped in unit 270", bytes(data)
