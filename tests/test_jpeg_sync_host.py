"""The self-synchronising entropy decoder (csrc/jpeg_sync.h) without a GPU: a stand-alone sanitizer build (its own ``main``, never
loaded into Python) runs the very inline functions ``entropy_kernel<1>`` runs, lanes and passes emulated by loops, at S and S / 2,
over valid files (coefficients and status equal to ``yv3_jpeg_decode_unit``'s, no unit handed over, PIL's pixels, and the proven
entry state of every subsequence equal to the state an independent bit-by-bit walk has at that bit), over inputs searched for
their subsequence boundaries, over crafted files and over damaged ones; and the ``_ex`` entry points' host checks."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_craft
from tests.jpeg_checkers import build_checker, run_checker
from tests.test_jpeg_host import HOST_CASES, PHOTO, encode, picture
from yolo_v3_amd import _ffi, jpeg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(REPO, "yolo_v3_amd", "csrc", "jpeg_sync.h")).read()
S = int(re.search(r"#define YV3_JPEG_SYNC_S (\d+)", _HEADER).group(1))
LANES = int(re.search(r"#define YV3_JPEG_SYNC_LANES (\d+)", _HEADER).group(1))
P = int(re.search(r"#define YV3_JPEG_SYNC_P (\d+)", _HEADER).group(1))
MIN_FACTOR = int(re.search(r"#define YV3_JPEG_SYNC_MIN_BYTES \((\d+) \* YV3_JPEG_SYNC_S\)", _HEADER).group(1))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker("jpeg_sync_host_check.cpp", tmp_path_factory.mktemp("jpeg_sync_host") / "jpeg_sync_host_check")


def scan_of(data):
    f = jpeg.parse(data)
    assert f.reason == 0
    return data[f.scan_offset:f.scan_offset + f.scan_length]


def check_valid(checker, tmp_path, data, name="", parallel=None):
    """``data`` through the parallel host decode at S and S / 2.  Returns the summary fields at S.  ``parallel``: whether some unit
    must (True) or cannot (False) have taken the parallel path at S."""
    (tmp_path / "in.jpg").write_bytes(data)
    ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    at_s = None
    for s in (S, S // 2):
        lines = run_checker(checker, "decode", tmp_path / "in.jpg", tmp_path / "out.rgb", s).splitlines()
        w = lines[0].split()
        f = dict(zip(w[0::2], (int(v) for v in w[1::2])))
        assert (f["reason"], f["status"], f["serial"], f["coef_equal"], f["handed"]) == (0, 0, 0, 1, 0), (name, s, lines[0])
        assert len(lines) - 1 == f["nsub"]
        for line in lines[1:]:
            v = line.split()                 # sub U I symbols 0|1 parallel bit blk zz serial bit blk zz
            par, ser = [int(x) for x in v[6:9]], [int(x) for x in v[10:13]]
            if par[0] == -2:                 # never committed: only a subsequence in which no symbol begins may be
                assert v[4] == "0", (name, s, line)
            else:
                assert par == ser, (name, s, line)
        head, _, px = (tmp_path / "out.rgb").read_bytes().partition(b"\n")
        assert head == b"%d %d" % (ref.shape[1], ref.shape[0]), (name, s)
        assert np.array_equal(np.frombuffer(px, np.uint8).reshape(ref.shape), ref), (name, s)
        if s == S:
            at_s = f
    if parallel is not None:
        assert (at_s["long_units"] > 0) == parallel, (name, at_s)
    return at_s


def table_files():
    """The five files of DESIGN.md section 8f's synchronisation table, the 1x1 file and the flat 64x48 file."""
    noise = picture(128, 96, seed=0)
    return [("photograph", open(PHOTO, "rb").read()),
            ("noise q75 4:2:0", encode(noise, quality=75, subsampling=2)),
            ("noise grey channel q50", encode(noise.split()[0], quality=50)),
            ("gradient q90 4:2:2", encode(picture(128, 96, kind="gradient"), quality=90, subsampling=1)),
            ("noise q100 4:4:4", encode(noise, quality=100, subsampling=0)),
            ("1x1", encode(picture(1, 1), quality=75)),
            ("flat 64x48", encode(picture(64, 48, kind="flat"), quality=75))]


@pytest.mark.parametrize("mode,subsampling,size,quality,optimize,restart", HOST_CASES)
def test_parallel_host_decode_of_the_host_cases(checker, tmp_path, mode, subsampling, size, quality, optimize, restart):
    kw = {"quality": quality, "optimize": optimize}
    if subsampling is not None:
        kw["subsampling"] = subsampling
    if restart == "rows":
        kw["restart_marker_rows"] = 1
    elif restart:
        kw["restart_marker_blocks"] = restart
    check_valid(checker, tmp_path, encode(picture(size[0], size[1], mode), **kw), str((mode, subsampling, size)))


@pytest.mark.parametrize("index", range(7))
def test_parallel_host_decode_of_the_table_files(checker, tmp_path, index):
    name, data = table_files()[index]
    f = check_valid(checker, tmp_path, data, name, parallel=index < 5)
    if index < 5:
        assert f["nsub"] == -(-f["scan_bytes"] // S) and f["windows"] >= -(-f["nsub"] // LANES)      # the photograph: two windows


def test_q100_noise_completes_within_the_bound_of_the_window_rule(checker, tmp_path):
    """The file that needs about 13 KB of scan to synchronise.  A window's first subsequence is proven and proving pass p proves
    subsequence p of the window at the latest, so a window of W lanes commits min(P + 1, W) subsequences or more (the last window
    what is left) in at most P proving passes: ceil(nsub / min(P + 1, W)) windows at the most, P passes each."""
    data = table_files()[4][1]
    (tmp_path / "in.jpg").write_bytes(data)
    n = len(scan_of(data))
    assert n > 40000
    for s in (S, S // 2):
        w = run_checker(checker, "decode", tmp_path / "in.jpg", tmp_path / "out.rgb", s).splitlines()[0].split()
        f = dict(zip(w[0::2], (int(v) for v in w[1::2])))
        nsub = -(-n // s)
        bound = P * -(-nsub // min(P + 1, LANES))
        print("S %d: %d subsequences, %d windows, %d proving passes (bound %d)" % (s, nsub, f["windows"], f["passes"], bound))
        assert (f["status"], f["handed"], f["coef_equal"], f["nsub"]) == (0, 0, 1, nsub)
        assert 0 < f["passes"] <= bound and f["windows"] <= -(-nsub // min(P + 1, LANES))


def find_boundary_files():
    """Noise files (no restart markers: the unit begins at byte 0 of the scan) searched, over seeds, for a given byte pattern
    around a multiple of S inside the scan; and files whose scan has a given length."""
    want = {"00 of a pair first": lambda sc, k: sc[k - 1] == 0xFF and sc[k] == 0,           # = its FF is the last byte before the cut
            "FF first": lambda sc, k: sc[k] == 0xFF,
            "pair ends at the cut": lambda sc, k: sc[k - 2] == 0xFF and sc[k - 1] == 0}
    found = {}
    for seed in range(400):
        data = encode(picture(48, 40, seed=seed), quality=97, subsampling=(0, 1, 2)[seed % 3])
        sc = scan_of(data)
        for name, hit in want.items():
            if name not in found and any(hit(sc, k) for k in range(S, len(sc) - 2, S)):
                found[name] = data
        if len(found) == len(want):
            break
    lengths = {}
    targets = [S - 1, S, S + 1, MIN_FACTOR * S - 1, MIN_FACTOR * S, MIN_FACTOR * S + 1, "multiple"]
    for seed in range(40):
        for w in range(8, 49, 4):
            for q in range(30, 99, 4):
                data = encode(picture(w, 16, "L", seed=seed), quality=q)
                n = len(scan_of(data))
                if n in targets and n not in lengths:
                    lengths[n] = data
                if n % S == 0 and n > MIN_FACTOR * S and "multiple" not in lengths:
                    lengths["multiple"] = data
        if len(lengths) == len(targets):
            break
    return found, want, lengths, targets


def test_subsequence_boundaries(checker, tmp_path):
    found, want, lengths, targets = find_boundary_files()
    assert set(found) == set(want), sorted(set(want) - set(found))
    assert set(lengths) == set(targets), [t for t in targets if t not in lengths]
    for name, data in found.items():
        check_valid(checker, tmp_path, data, name, parallel=True)
    for n, data in lengths.items():
        check_valid(checker, tmp_path, data, "scan of %s bytes" % n, parallel=(n == "multiple" or n >= MIN_FACTOR * S))


def crafted_long_files():
    """`jpeg_craft`'s families at sizes whose units are long enough for the parallel path."""
    rng = np.random.RandomState(31)
    out = []
    long_codes = dict(jpeg_craft._std())
    long_codes[(1, 0)] = ([1] + [0] * 14 + [255], list(range(256)))
    out.append(jpeg_craft._grey("16-bit codes", 160, 96, jpeg_craft._ordinary(rng, 12, 20), huff=long_codes))
    c = np.zeros((12, 20, 64), np.int64)
    c[..., 0] = rng.randint(-40, 41, (12, 20))
    for k in (16, 32, 48, 63):
        c[..., jpeg_craft.NATURAL_OF_ZIGZAG[k]] = rng.choice([-6, -3, -1, 1, 2, 5], (12, 20))
    out.append(jpeg_craft._grey("zrl chains", 160, 96, c))
    c = np.zeros((12, 20, 64), np.int64)
    c[..., jpeg_craft.NATURAL_OF_ZIGZAG[63]] = rng.choice([-2, 1], (12, 20))       # ZRL ZRL ZRL and one coefficient: no EOB
    out.append(jpeg_craft._grey("zrl to 63", 160, 96, c))
    c = np.zeros((16, 24, 64), np.int64)
    c[..., 0] = np.where((np.arange(16)[:, None] + np.arange(24)[None, :]) % 2 == 0, 1016, -1024)
    out.append(jpeg_craft._grey("dc category 11", 192, 128, c, q=[1] * 64))
    c = np.zeros((12, 20, 64), np.int64)                          # seventeen one-bits in a row in every block: an FF 00 pair each
    c[..., 0] = rng.randint(-40, 41, (12, 20))
    c[..., jpeg_craft.NATURAL_OF_ZIGZAG[1]] = c[..., jpeg_craft.NATURAL_OF_ZIGZAG[2]] = 255
    name, data = jpeg_craft._grey("stuffed bytes", 160, 96, c, q=[1] * 64)
    sc = scan_of(data)
    assert sum(sc[k - 1] == 0xFF and sc[k] == 0 for k in range(S // 2, len(sc), S // 2)) >= 3        # pairs cut in two
    out.append((name, data))
    huff = jpeg_craft._std(luma_dc=(2, 3), chroma_dc=(1, 0), luma_ac=(3, 2), chroma_ac=(0, 1))
    quant = {i: rng.randint(1, 9, 64) for i in range(4)}
    for (h, v) in ((1, 1), (2, 1), (2, 2)):
        mw, mh = (101 + 8 * h - 1) // (8 * h), (77 + 8 * v - 1) // (8 * v)
        comps = [jpeg_craft.Component(jpeg_craft._ordinary(rng, mh * v, mw * h), h, v, tq=2, td=2, ta=3),
                 jpeg_craft.Component(jpeg_craft._ordinary(rng, mh, mw), 1, 1, tq=3, td=1, ta=0),
                 jpeg_craft.Component(jpeg_craft._ordinary(rng, mh, mw), 1, 1, tq=0, td=3, ta=2)]
        out.append(("selectors 2 and 3 %dx%d" % (h, v), jpeg_craft.write(101, 77, comps, quant, huff, ids=(7, 200, 0), sof=1)))
    out.append(segments_300(rng, (5, 250)))
    return out


def segments_300(rng, long_units):
    """300 restart segments of four blocks: flat ones of a few bytes, and those of ``long_units`` of noise at q = 1 (hundreds of
    bytes each)."""
    c = np.zeros((1200, 1, 64), np.int64)
    c[:, 0, 0] = rng.randint(-40, 41, 1200)
    for unit in long_units:
        c[4 * unit:4 * unit + 4] = jpeg_craft.encodable(rng.randint(0, 256, (32, 8)), 1)
    return jpeg_craft._grey("300 segments, two long", 8, 9600, c, q=[1] * 64, restart=4)


def test_crafted_files(checker, tmp_path):
    for name, data in crafted_long_files():
        f = check_valid(checker, tmp_path, data, name, parallel=True)
        if name.startswith("300"):
            assert (f["units"], f["long_units"]) == (300, 2)
    for name, data in jpeg_craft.family_a():                     # the family as it is (most of its units are short ones)
        check_valid(checker, tmp_path, data, name)


@pytest.mark.parametrize("group", ["rounds", "window_edges", "cuts", "dc_shapes"])
def test_gpu_case_files_are_what_their_names_say(checker, tmp_path, group):
    """The files of tests/jpeg_sync_cases.py, which test_gpu_jpeg_sync gives to the kernel: each decodes (PIL's pixels, through
    `check_valid`) and still has the property it is in the batch for."""
    from tests import jpeg_sync_cases as cases
    files = getattr(cases, group)()
    assert len(files) == len({n for n, _ in files}) >= 4
    for name, data in files:
        want = cases.EXPECT[name]
        f = check_valid(checker, tmp_path, data, name, parallel=want["long_units"] > 0)
        for key in ("units", "long_units", "nsub", "scan_bytes"):
            if key in want:
                assert f[key] == want[key], "%s: %s is %d, meant to be %d" % (name, key, f[key], want[key])
        assert len(want["long_at"]) == want["long_units"], "%s: %d long units counted in the file" % (name, len(want["long_at"]))
        for key in ("per_round", "long_at"):
            if key + "_meant" in want:
                assert want[key] == want[key + "_meant"], "%s: %s is %s, meant to be %s" % (name, key, want[key], want[key + "_meant"])
        if "mcus" in want:
            w, h = Image.open(io.BytesIO(data)).size
            assert (f["units"], -(-w // 8) * -(-h // 8)) == (1, want["mcus"]), "%s: not one unit of %d MCUs" % (name, want["mcus"])
        ceil = -(-f["nsub"] // LANES)
        rule = {None: True, "1": f["windows"] == 1, ">=2": f["windows"] >= 2, ">ceil": f["windows"] > ceil}[want.get("windows")]
        assert rule, "%s: %d windows for %d subsequences, meant to be %s" % (name, f["windows"], f["nsub"], want["windows"])


def test_gpu_case_file_damaged_in_round_two_hands_a_unit_over(checker, tmp_path):
    """The bit flipped in unit 270 is an error the lanes meet from a proven state (no marker that the first look at the unit
    finds): one unit handed over, and the serial routine's status."""
    from tests import jpeg_sync_cases as cases
    name, data = cases.damaged_round_two()
    assert jpeg.parse(data).reason == 0 and len(cases.unit_lengths(data)) == 300
    (tmp_path / "in.jpg").write_bytes(data)
    w = run_checker(checker, "decode", tmp_path / "in.jpg", tmp_path / "out.rgb", S).splitlines()[0].split()
    f = dict(zip(w[0::2], (int(v) for v in w[1::2])))
    assert f["status"] == f["serial"] != 0 and f["handed"] == 1 and (f["units"], f["long_units"]) == (300, 300), (name, f)


@pytest.mark.parametrize("kw", [dict(subsampling=2, restart_marker_blocks=2), dict(subsampling=1, optimize=True), dict(subsampling=0)])
def test_damaged_inputs_get_the_serial_status(checker, tmp_path, kw):
    """Every prefix truncation, 2000 seeded single-byte corruptions and 500 random tails of a small file, at S and S / 2, under
    ASan + UBSan: the parallel path's status is the serial one's, and so are its coefficients wherever that status is 0."""
    data = encode(picture(33, 19, seed=3), quality=75, **kw)
    (tmp_path / "in.jpg").write_bytes(data)
    w = run_checker(checker, "fuzz", tmp_path / "in.jpg", 7).split()
    f = dict(zip(w[0::2], (int(v) for v in w[1::2])))
    print(f)
    assert f["inputs"] == 2 * (len(data) + 2500) and f["mismatches"] == 0
    assert f["ok"] > 0 and f["errors"] > 0 and f["long_units"] > 0 and f["handed"] > 0         # every kind of outcome was met


# ---- the C interface, no GPU -------------------------------------------------------------------------------------------------------
def test_ex_entry_points_check_their_arguments_before_launching():
    """Dummy device pointers, as in test_jpeg_host: every answer comes from the host checks, so nothing is launched."""
    lib = _ffi.lib()
    infos = (_ffi.JpegInfo * 2)()
    infos[0] = jpeg.parse(encode(picture(33, 19), subsampling=2))
    infos[1] = jpeg.parse(encode(picture(7, 9, "L")))
    host = ctypes.addressof(infos)
    need = lib.yv3_jpeg_workspace_bytes(host, 2)
    assert need == 256 + (36 * 128 + 36 * 64 + 256) + (2 * 128 + 256 + 256)
    assert lib.yv3_jpeg_workspace_bytes_ex(host, 2, 0) == need and lib.yv3_jpeg_workspace_bytes_ex(host, 2, 1) == need
    assert lib.yv3_jpeg_workspace_bytes_ex(host, 2, 2) == 0 and lib.yv3_jpeg_workspace_bytes_ex(host, 2, -1) == 0
    assert lib.yv3_jpeg_workspace_bytes_ex(None, 2, 1) == 0 and lib.yv3_jpeg_workspace_bytes_ex(host, 0, 1) == 0

    def desc(**kw):
        d = _ffi.JpegBatchDesc(src=4096, src_bytes=1000, src_offsets=4096, infos=4096, infos_host=host, dst=4096, dst_bytes=5000,
                               dst_offsets=4096, status=4096, B=2)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    for entropy in (0, 1):
        for handed in (None, 4096):
            call = lambda d, ws, n: lib.yv3_jpeg_decode_batch_ex(d, entropy, handed, ws, n, None)
            assert call(desc(), 4096, need - 1) == _ffi.EWORKSPACE
            assert call(None, 4096, need - 1) == _ffi.EINVAL
            assert call(desc(B=0), None, need - 1) == _ffi.EINVAL
            for field in ("src", "src_offsets", "infos", "infos_host", "dst", "dst_offsets", "status"):
                assert call(desc(**{field: None}), 4096, need - 1) == _ffi.EINVAL, field
            assert call(desc(), 4096 + 8, need - 1) == _ffi.EINVAL
            for field, value in (("B", 0), ("B", 65536), ("src_bytes", 0), ("dst_bytes", -1)):
                assert call(desc(**{field: value}), 4096, 1 << 40) == _ffi.EINVAL, field
            refused = (_ffi.JpegInfo * 2)()
            refused[0], refused[1] = infos[0], jpeg.parse(encode(picture(33, 19), progressive=True))
            assert call(desc(infos_host=ctypes.addressof(refused)), 4096, 1 << 40) == _ffi.ESHAPE
    for entropy in (2, -1):                                       # (with a workspace one byte short, like every call above)
        assert lib.yv3_jpeg_decode_batch_ex(desc(), entropy, None, 4096, need - 1, None) == _ffi.EINVAL


def test_ctypes_mirrors_match_the_header(tmp_path):
    """A C compiler takes the header's prototypes for the signatures `_ffi` declares, and the selectors are 0 and 1."""
    src = tmp_path / "proto.c"
    src.write_text('#include <stddef.h>\n#include "yv3.h"\n'
                   "size_t (*a)(const yv3_jpeg_info*, int, int) = yv3_jpeg_workspace_bytes_ex;\n"
                   "int (*b)(const yv3_jpeg_batch_desc*, int, int*, void*, size_t, void*) = yv3_jpeg_decode_batch_ex;\n")
    subprocess.run(["cc", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "proto.o")], check=True)
    src = tmp_path / "enum.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv3.h"\n'
                   'int main(void){printf("%d %d", YV3_JPEG_ENTROPY_SERIAL, YV3_JPEG_ENTROPY_PARALLEL); return 0;}\n')
    subprocess.run(["cc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "enum")], check=True)
    out = subprocess.run([str(tmp_path / "enum")], capture_output=True, text=True, check=True).stdout.split()
    assert [int(v) for v in out] == [jpeg.ENTROPY["serial"], jpeg.ENTROPY["parallel"]] == [0, 1]
    c_int, c_void_p, c_size_t = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
    lib = _ffi.lib()
    assert lib.yv3_jpeg_workspace_bytes_ex.restype is c_size_t and lib.yv3_jpeg_workspace_bytes_ex.argtypes == [c_void_p, c_int, c_int]
    assert lib.yv3_jpeg_decode_batch_ex.restype is c_int
    assert lib.yv3_jpeg_decode_batch_ex.argtypes == [ctypes.POINTER(_ffi.JpegBatchDesc), c_int, c_void_p, c_void_p, c_size_t, c_void_p]
    header = open(os.path.join(REPO, "include", "yv3.h")).read()
    assert len(re.findall(r"#define YV3_(JPEG_[A-Z_]+)\s+(\d+)", header)) == 22       # the selectors are an enum, not codes
    with pytest.raises(ValueError):
        jpeg.decode_batch([], entropy="fast")
