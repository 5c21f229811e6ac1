"""Host-only run of DescKind::Stats, the validator arm tensor_stats uses:
tests/native/desc_check_stats_selftest.cpp is compiled with ASan + UBSan by
the host compiler and run directly, with no HIP call anywhere in the
program. Nothing is loaded into Python under a sanitizer."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "desc_check_stats_selftest.cpp")
INCLUDE = os.path.join(REPO, "torchsnapshot_amd", "ops", "hip")


def test_desc_check_stats_under_asan_ubsan(tmp_path):
    names = (os.environ.get("CXX"), "g++", "clang++", "c++")
    cxx = next((shutil.which(n) for n in names if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "desc_check_stats_selftest")
    flags = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer",
             "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    build = subprocess.run(
        [cxx, *flags, f"-I{INCLUDE}", SRC, "-o", exe], capture_output=True, text=True
    )
    if build.returncode != 0 and any(
        word in build.stderr.lower() for word in ("asan", "ubsan", "sanitize")
    ):
        pytest.skip("host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "desc_check stats selftest OK" in run.stdout
