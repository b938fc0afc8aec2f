"""csrc/device_mem.hpp (the owners of the context's device memory) on the host: tests/host/device_mem_test.cpp instantiates
both types on a malloc-backed policy and runs under AddressSanitizer and UndefinedBehaviorSanitizer as a child process of its
own.  No GPU is opened, nothing is loaded into this interpreter."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "host", "device_mem_test.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def _compilers():
    """Host C++ compilers to try, as command prefixes: ROCm's clang++ (its sanitizer runtime is linked statically), g++, hipcc."""
    out = []
    for exe in (shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", shutil.which("g++")):
        if exe and os.path.exists(exe) and [exe] not in out:
            out.append([exe])
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc):
        out.append([hipcc, "-x", "c++"])
    return out


def _sanitizing_compiler(tmp):
    """The first compiler that builds AND runs a trivial program with -fsanitize=address, or None."""
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    for cc in _compilers():
        exe = os.path.join(tmp, "probe")
        r = subprocess.run(cc + ["-fsanitize=address", probe, "-o", exe], capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([exe], capture_output=True).returncode == 0:
            return cc
    return None


def test_device_mem_types_under_sanitizers(tmp_path):
    cc = _sanitizing_compiler(str(tmp_path))
    if cc is None:
        pytest.skip("no C++ compiler on this machine links -fsanitize=address")
    exe = str(tmp_path / "device_mem_test")
    build = subprocess.run(cc + ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + SANITIZE + [SOURCE, "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout + run.stderr
    assert run.returncode == 0, out
    assert "device_mem host test OK" in run.stdout, out
    assert "runtime error" not in out and "Sanitizer" not in out, out
