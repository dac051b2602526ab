"""The owners of device memory (graphite_amd/csrc/gg_devmem.h: the arena, the
growable buffer and the grouped growth — plain host C++ over a replaceable
allocator) under AddressSanitizer and UBSan on the CPU: tools/devmem_check/
devmem_check.cpp is a stand-alone program that substitutes a counting
allocator and makes its k-th call fail, on first growth and on regrowth, and
checks that no block leaks or is freed twice.  It is compiled here with the
host compiler and run as a child process; nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "devmem_check", "devmem_check.cpp")


def test_devmem_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler on PATH")
    exe = str(tmp_path / "devmem_check")
    # (the runtimes linked statically where the compiler has the switch: g++)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-Wall", "-Wextra", "-Werror", SRC, "-o", exe] + static
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0 and ("asan" in b.stdout.lower() or "ubsan" in b.stdout.lower() or "sanitize" in b.stdout.lower()):
        pytest.skip("the host toolchain cannot link the sanitizer runtime: %s" % b.stdout.strip().splitlines()[-1])
    assert b.returncode == 0, b.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "devmem_check: ok" in r.stdout
