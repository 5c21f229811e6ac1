"""Host-only run of the descriptor validator: ops/hip/desc_check.h is plain
C++, so a stand-alone program (tests/native/desc_check_selftest.cpp) is
compiled with ASan + UBSan by the host compiler and run directly. It feeds
check_descs one bad descriptor per rule for each entry point - the capped
gather size and a misaligned plain-gather base among them - with no HIP
call anywhere in the program. Nothing is loaded into Python under a
sanitizer."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "desc_check_selftest.cpp")
INCLUDE = os.path.join(REPO, "torchsnapshot_amd", "ops", "hip")


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_desc_check_under_asan_ubsan(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "desc_check_selftest")
    build = subprocess.run(
        [
            cxx,
            "-std=c++17",
            "-O1",
            "-g",
            "-fno-omit-frame-pointer",
            "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all",
            f"-I{INCLUDE}",
            SRC,
            "-o",
            exe,
        ],
        capture_output=True,
        text=True,
    )
    if build.returncode != 0 and any(
        word in build.stderr.lower() for word in ("asan", "ubsan", "sanitize")
    ):
        # e.g. "cannot find -lasan": compiler present, runtime not installed
        pytest.skip("host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "desc_check selftest OK" in run.stdout

