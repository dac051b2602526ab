"""The reader of a windowed run's `win` snapshot section (graphite_amd/csrc/
gg_snapshot_win.h, what gg_window_snapshot_state calls: plain host C++ over
bytes that may come from a file) under AddressSanitizer and UBSan on the CPU.
tools/snapshot_check/window_check.cpp is a stand-alone program that builds
containers with ggsnap::Layout in exact-size heap blocks — a valid win
section, none, one of the wrong size for num_tiles, num_tiles = 0, a truncated
table, a section past the buffer, a bad checksum — and checks each verdict and
each filled array.  It is compiled here with the host compiler and run as a
child process; nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "snapshot_check", "window_check.cpp")


def test_window_section_reader_under_sanitizers(tmp_path):
    assert os.path.exists(SRC), "tools/snapshot_check/window_check.cpp is missing"
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler on PATH")
    exe = str(tmp_path / "window_check")
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
    assert "window_check: ok" in r.stdout
