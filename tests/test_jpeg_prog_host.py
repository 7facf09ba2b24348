"""The host half of progressive JPEG decode (csrc/jpeg_parse.cpp's yv3_jpeg_parse_ex, csrc/jpeg_prog.h), without a GPU: a
stand-alone sanitizer build (tests/jpeg_prog_host_check.cpp: its own ``main``, never loaded into Python) runs the parser, the
entropy routine level by level and the existing IDCT and pixel code over PIL-written files, crafted scripts, refused scripts and
damaged files, every result against PIL on the same bytes, bit for bit; plus the contract with the older entry points, the ctypes
mirrors against the header and the argument checks that answer before any launch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import jpeg_checkers
from tests import jpeg_prog_craft as craft
from tests.jpeg_checkers import run_checker
from yolo_v3_amd import _ffi, jpeg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_checker(out, sanitize):
    """tests/jpeg_prog_host_check.cpp as the program ``out`` (the GPU tests build it without the sanitizers, for its statuses)."""
    return jpeg_checkers.build_checker("jpeg_prog_host_check.cpp", out, sanitize)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return build_checker(tmp_path_factory.mktemp("jpeg_prog_host") / "jpeg_prog_host_check", sanitize=True)


def host_decode(checker, tmp_path, files):
    """[(reason, accepted, status, levels, pixels or None)] of the host program for each of ``files``, in one run."""
    args = []
    for i, data in enumerate(files):
        (tmp_path / ("%d.jpg" % i)).write_bytes(data)
        if (tmp_path / ("%d.rgb" % i)).exists():
            (tmp_path / ("%d.rgb" % i)).unlink()
        args += [tmp_path / ("%d.jpg" % i), tmp_path / ("%d.rgb" % i)]
    lines = run_checker(checker, "decode", *args).strip().splitlines()
    assert len(lines) == len(files)
    out = []
    for i, line in enumerate(lines):
        w = line.split()
        reason, accepted, status, levels = int(w[1]), int(w[3]), int(w[5]), int(w[7])
        px = None
        if (reason == 0 or accepted) and status == 0:
            head, _, body = (tmp_path / ("%d.rgb" % i)).read_bytes().partition(b"\n")
            width, height = (int(v) for v in head.split())
            px = np.frombuffer(body, np.uint8).reshape(height, width, 3)
        out.append((reason, accepted, status, levels, px))
    return out


def check_valid(checker, tmp_path, family):
    """No exceptions: every file of the family is accepted, decodes at status 0 to PIL's pixels and to its baseline twin's."""
    got = host_decode(checker, tmp_path, [f for _, f, _ in family] + [t for _, _, t in family])
    n = len(family)
    for i, (name, data, twin) in enumerate(family):
        reason, accepted, status, levels, px = got[i]
        assert (reason, accepted, status) == (_ffi.JPEG_PROGRESSIVE, 1, 0), name
        ref = craft.pil_pixels(data)
        assert px.shape == ref.shape and np.array_equal(px, ref), name
        assert got[n + i][:3] == (0, 0, 0) and np.array_equal(got[n + i][4], px), name          # the baseline decoder on the twin
    return got[:n]


def test_pil_written_files_equal_pil_and_their_baseline_twins(checker, tmp_path):
    family = craft.valid_files()
    assert len(family) == 4 * 7 * 3 * 2 * 3
    got = check_valid(checker, tmp_path, family)
    assert {g[3] for g in got} == {3}                                   # PIL's scripts have three levels


def test_crafted_scripts_equal_pil_and_their_baseline_twins(checker, tmp_path):
    family = craft.crafted()
    got = dict(zip([name for name, _, _ in family], check_valid(checker, tmp_path, family)))
    assert got["spectral selection only"][3] == 1 and got["al 3, three refinements"][3] == 4
    assert got["64 scans"][3] == 8                                      # 64 tables, eight to a level
    by_name = {name: data for name, data, _ in family}
    info, prog = jpeg.parse_ex(by_name["64 scans"])
    assert (prog.nscans, prog.ntables) == (64, 64)
    info, prog = jpeg.parse_ex(by_name["more units than lanes"])
    assert prog.nlevels == 1 and all(prog.scans[i].restart_interval == 1 for i in range(3))          # 900 units in one level
    info, prog = jpeg.parse_ex(by_name["a restart interval per scan"])
    assert [prog.scans[i].restart_interval for i in range(10)] == [2, 0, 1, 5, 3, 7, 1, 0, 2, 4]
    assert [prog.scans[i].level for i in range(10)] == [1, 1, 1, 1, 1, 2, 2, 2, 2, 3]
    # the EOB14 code is in the file: the first AC scan's table holds symbol 0xE0
    info, prog = jpeg.parse_ex(by_name["eob14 across block rows"])
    assert 0xE0 in list(prog.tables[prog.scans[1].tab[0]].values)[:sum(prog.tables[prog.scans[1].tab[0]].counts)]


def test_refused_scripts_carry_their_reason(checker, tmp_path):
    family = craft.refused_scripts()
    assert len(family) == 8
    got = host_decode(checker, tmp_path, [data for _, data, _ in family])
    for (name, data, reason), g in zip(family, got):
        info, prog = jpeg.parse_ex(data)
        assert prog is None and info.reason == getattr(_ffi, reason) and info.reason > 11, name
        assert g[:3] == (info.reason, 0, 0), name
        assert jpeg.parse(data).reason == _ffi.JPEG_PROGRESSIVE, name
        assert not jpeg.Source(data, progressive=True).on_gpu or jpeg.Source(data, progressive=True).error is not None, name


@pytest.mark.parametrize("which", [0, 1, 2])
def test_damaged_inputs_end_in_a_reason_or_a_status_under_the_sanitizers(checker, tmp_path, which):
    """Every prefix truncation, 2000 seeded single-byte corruptions of the scan data and 300 of the headers, each on an exact-size
    heap copy and decoded through the IDCT to its pixels: a clean exit, and a (reason, accepted, status) for every input.  The
    program cannot ask PIL: the pixels of the inputs that end at status 0 are compared with PIL's for the 300 seeded corruptions of
    `test_corruptions_that_decode_are_pils_pixels` and for the prefix truncations below, not for these 2300."""
    name, data = craft.damage_sources()[which]
    (tmp_path / "in.jpg").write_bytes(data)
    lines = run_checker(checker, "fuzz", tmp_path / "in.jpg", 7).strip().splitlines()
    assert lines[0] == "inputs %d" % (len(data) + 2300)
    seen = {tuple(int(v) for v in l.split()[1:6:2]): int(l.split()[7]) for l in lines[1:]}
    assert sum(seen.values()) == len(data) + 2300
    for reason, accepted, status in seen:
        assert 0 <= reason <= 15 and 0 <= status <= 12
        assert accepted == (reason == _ffi.JPEG_PROGRESSIVE)            # with the flag, reason 3 is the accepted file's alone
        assert not status or accepted or reason == 0
    assert (_ffi.JPEG_PROGRESSIVE, 1, 0) in seen and (_ffi.JPEG_PROGRESSIVE, 1, _ffi.JPEG_S_OVERRUN) in seen
    assert any(r > 11 for r, _, _ in seen) and {s for _, _, s in seen} & {_ffi.JPEG_S_CODE, _ffi.JPEG_S_COEF}
    # every prefix truncation again, through the decode mode: whichever ends at status 0 holds PIL's pixels of the same bytes, or
    # is a file whose last scan runs to its end, which PIL refuses and `jpeg.Source` marks
    cuts = [data[:n] for n in range(len(data))]
    decoded = 0
    for f, (reason, accepted, status, _, px) in zip(cuts, host_decode(checker, tmp_path, cuts)):
        if accepted and status == 0:
            decoded += 1
            ref = craft.pil_pixels(f)
            if ref is None:                                             # PIL raises on a file without EOI: `jpeg` calls it truncated
                assert jpeg.Source(f, progressive=True).unterminated, len(f)
            else:
                assert ref.shape == px.shape and np.array_equal(ref, px), len(f)
    assert decoded >= 1                                                 # the file without its EOI, at least


# Of 300 seeded corruptions of the scan data (`craft.corruptions`, seeds `craft.DAMAGE_SEEDS`), these many decode at status 0 on
# the host; each of them must then be PIL's pixels.  The floor is half of each.
STATUS0_MEASURED = {"420 33x19 q75": 60, "444 24x16 q95 restarts": 58, "grey 40x24 q50": 72}


@pytest.mark.parametrize("which", [0, 1, 2])
def test_corruptions_that_decode_are_pils_pixels(checker, tmp_path, which):
    name, data = craft.damage_sources()[which]
    files = craft.corruptions(data, 300, craft.DAMAGE_SEEDS[which])
    got = host_decode(checker, tmp_path, files)
    decoded = 0
    for f, (reason, accepted, status, _, px) in zip(files, got):
        if accepted and status == 0:
            decoded += 1
            ref = craft.pil_pixels(f)
            assert ref is not None and ref.shape == px.shape and np.array_equal(ref, px)
    print("status 0:", name, decoded)
    assert decoded >= STATUS0_MEASURED[name] // 2 and decoded >= 1
    assert decoded < 300                                                # at least one corruption is refused


def test_contract_with_the_old_entries():
    """yv3_jpeg_parse == yv3_jpeg_parse_ex(accept = 0) on every file of the families, twins included; an accepted progressive file's
    info record is refused by every older entry point."""
    lib = _ffi.lib()
    files = [f for _, f, _ in craft.valid_files()] + [t for _, _, t in craft.valid_files()] + [t for _, _, t in craft.crafted()]
    files += [f for _, f, _ in craft.crafted()] + [f for _, f, _ in craft.refused_scripts()] + [f for _, f in craft.damage_sources()]
    files += [b"", b"\xff\xd8", files[0][:100], files[3][:-30]]
    for data in files:
        old, new, prog = _ffi.JpegInfo(), _ffi.JpegInfo(), _ffi.JpegProg()
        assert lib.yv3_jpeg_parse(data, len(data), ctypes.byref(old)) == 0
        assert lib.yv3_jpeg_parse_ex(data, len(data), 0, ctypes.byref(new), ctypes.byref(prog)) == 0
        assert bytes(old) == bytes(new) and bytes(prog) == bytes(ctypes.sizeof(prog))
        assert lib.yv3_jpeg_parse_ex(data, len(data), 0, ctypes.byref(new), None) == 0 and bytes(old) == bytes(new)
    refused = jpeg.parse(b"\x89PNG\r\n\x1a\n" + bytes(64))
    for _, data, _ in craft.crafted()[:3] + craft.valid_files()[:2]:
        info, prog = jpeg.parse_ex(data)
        assert prog is not None and info.reason == _ffi.JPEG_PROGRESSIVE
        # the record adds nothing to a workspace: what is left is the slot table of B = 1, as for any refused record
        assert lib.yv3_jpeg_workspace_bytes(ctypes.byref(info), 1) == 256 == lib.yv3_jpeg_workspace_bytes(ctypes.byref(refused), 1)
        assert lib.yv3_jpeg_workspace_bytes_ex(ctypes.byref(info), 1, 0) == 256
        d = _ffi.JpegBatchDesc(src=4096, src_bytes=1000, src_offsets=4096, infos=4096, infos_host=ctypes.addressof(info), dst=4096,
                               dst_bytes=1 << 30, dst_offsets=4096, status=4096, B=1)
        assert lib.yv3_jpeg_decode_batch(ctypes.byref(d), 4096, 1 << 40, None) == _ffi.ESHAPE
        assert lib.yv3_jpeg_decode_batch_ex(ctypes.byref(d), 1, None, 4096, 1 << 40, None) == _ffi.ESHAPE
    info = _ffi.JpegInfo()
    assert lib.yv3_jpeg_parse_ex(b"", 0, 2, ctypes.byref(info), ctypes.byref(_ffi.JpegProg())) == _ffi.EINVAL
    assert lib.yv3_jpeg_parse_ex(b"", 0, 1, ctypes.byref(info), None) == _ffi.EINVAL


def test_decode_batch_prog_checks_its_arguments_before_launching():
    """Dummy device pointers: every answer comes from the host checks, so nothing is launched (and no GPU is needed)."""
    lib = _ffi.lib()
    data = craft.valid_files()[200][1]
    infos, progs, prog_of = (_ffi.JpegInfo * 2)(), (_ffi.JpegProg * 1)(), (ctypes.c_int * 2)(0, -1)
    infos[0], progs[0] = jpeg.parse_ex(data)
    infos[1] = jpeg.parse(craft.valid_files()[200][2])
    host = (ctypes.addressof(infos), ctypes.addressof(prog_of), ctypes.addressof(progs))
    need = lib.yv3_jpeg_workspace_bytes_prog(host[0], host[1], host[2], 1, 2, 0)
    assert need > lib.yv3_jpeg_workspace_bytes(ctypes.addressof(infos) + ctypes.sizeof(_ffi.JpegInfo), 1) > 0
    assert lib.yv3_jpeg_workspace_bytes_prog(host[0] + ctypes.sizeof(_ffi.JpegInfo), None, None, 0, 1, 0) == \
        lib.yv3_jpeg_workspace_bytes(host[0] + ctypes.sizeof(_ffi.JpegInfo), 1)
    assert lib.yv3_jpeg_workspace_bytes_prog(host[0], host[1], host[2], 1, 2, 7) == 0

    def desc(**kw):
        base = _ffi.JpegBatchDesc(src=4096, src_bytes=100000, src_offsets=4096, infos=4096, infos_host=host[0], dst=4096, dst_bytes=1 << 20,
                                  dst_offsets=4096, status=4096, B=2)
        d = _ffi.JpegBatchDescProg(base=base, progs=4096, progs_host=host[2], prog_of=4096, prog_of_host=host[1], P=1)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    call = lib.yv3_jpeg_decode_batch_prog
    assert call(ctypes.byref(desc()), 0, None, 4096, need - 1, None) == _ffi.EWORKSPACE
    assert call(None, 0, None, 4096, need - 1, None) == _ffi.EINVAL
    assert call(ctypes.byref(desc()), 5, None, 4096, need - 1, None) == _ffi.EINVAL
    assert call(ctypes.byref(desc()), 0, None, 4096 + 8, need - 1, None) == _ffi.EINVAL
    for field in ("progs", "progs_host", "prog_of", "prog_of_host"):
        assert call(ctypes.byref(desc(**{field: None})), 0, None, 4096, need - 1, None) == _ffi.EINVAL, field
    bad = (ctypes.c_int * 2)(1, -1)                                      # an index past P; a progressive record for a baseline image
    assert call(ctypes.byref(desc(prog_of_host=ctypes.addressof(bad))), 0, None, 4096, 1 << 40, None) == _ffi.ESHAPE
    bad = (ctypes.c_int * 2)(-1, -1)
    assert call(ctypes.byref(desc(prog_of_host=ctypes.addressof(bad))), 0, None, 4096, 1 << 40, None) == _ffi.ESHAPE
    bad = (ctypes.c_int * 2)(0, 0)
    assert call(ctypes.byref(desc(prog_of_host=ctypes.addressof(bad))), 0, None, 4096, 1 << 40, None) == _ffi.ESHAPE
    broken = (_ffi.JpegProg * 1)()
    broken[0] = progs[0]
    broken[0].scans[1].se = 64
    assert call(ctypes.byref(desc(progs_host=ctypes.addressof(broken))), 0, None, 4096, 1 << 40, None) == _ffi.ESHAPE


@pytest.mark.parametrize("ctype,cname", [(_ffi.JpegpScan, "yv3_jpegp_scan"), (_ffi.JpegpTable, "yv3_jpegp_table"),
                                         (_ffi.JpegProg, "yv3_jpeg_prog"), (_ffi.JpegBatchDescProg, "yv3_jpeg_batch_desc_prog")])
def test_struct_layouts_match_the_c_header(tmp_path, ctype, cname):
    fields = [f for f, _ in ctype._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yv3.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % cname
                   + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (cname, f) for f in fields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(ctype)] + [getattr(ctype, f).offset for f in fields]


def test_ffi_names_the_header_codes_and_the_library_the_entries():
    header = open(os.path.join(REPO, "include", "yv3.h")).read()
    codes = {n: int(v) for n, v in re.findall(r"#define YV3_(JPEGP_[A-Z_]+)\s+(\d+)", header)}
    assert len(codes) == 9 and codes == {n: v for n, v in vars(_ffi).items() if n.startswith("JPEGP_")}
    exported = subprocess.run(["nm", "-D", "--defined-only", _ffi.lib()._name], capture_output=True, text=True, check=True).stdout
    for name in ("yv3_jpeg_parse_ex", "yv3_jpeg_workspace_bytes_prog", "yv3_jpeg_decode_batch_prog", "yv3_jpeg_launch_count"):
        assert re.search(r"\bT %s\b" % name, exported) and re.search(r"\b%s\(" % name, header), name


def test_the_switch_is_off_by_default():
    data = craft.valid_files()[100][1]
    src = jpeg.Source(data)
    assert src.prog is None and not src.on_gpu and src.info.reason == _ffi.JPEG_PROGRESSIVE
    src = jpeg.Source(data, progressive=True)
    assert src.prog is not None and src.on_gpu and src.info.reason == _ffi.JPEG_PROGRESSIVE and not src.unterminated
    assert jpeg.Source(data[:-2], progressive=True).unterminated
