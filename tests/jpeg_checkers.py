"""Building and running the stand-alone JPEG host programs of tests/ (jpeg_host_check.cpp, jpeg_sync_host_check.cpp,
jpeg_prog_host_check.cpp): each has its own ``main`` and runs as a process of its own, never loaded into Python."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_checker(source_name, out, sanitize=True):
    """Compiles tests/``source_name`` to the program ``out`` and returns its path; with ``sanitize`` under ASan + UBSan (the CPU
    tests), without as a plain program (what a GPU test may build and run where it runs)."""
    cxx = shutil.which("c++")
    cmd = [cxx] if cxx else ["/opt/rocm/bin/hipcc", "-x", "c++"]
    if sanitize:
        # the sanitizer runtimes are linked statically (clang's default; gcc needs the flags): the program then runs in any environment
        if cxx and b"Free Software Foundation" in subprocess.run([cxx, "--version"], capture_output=True).stdout:
            cmd += ["-static-libasan", "-static-libubsan"]
        cmd += ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd + ["-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "yolo_v3_amd", "csrc"),
                          os.path.join(REPO, "tests", source_name), "-o", str(out)], check=True)
    return str(out)


def run_checker(checker, *args):
    """The program's standard output; a clean exit and no sanitizer report are asserted."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([checker] + [str(a) for a in args], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout
