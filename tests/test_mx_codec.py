"""The block-scaled codec (ops/hip/mx_codec.h) on the host:
tests/native/mx_codec_selftest.cpp holds block exponent, encode and decode of
both formats to a floating-point reference of its own, built with ASan + UBSan
by the host compiler and run directly. No HIP; nothing is loaded into Python."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mx_codec_under_asan_ubsan(tmp_path):
    names = (os.environ.get("CXX"), "g++", "clang++", "c++")
    cxx = next((shutil.which(n) for n in names if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "selftest")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", f"-I{REPO}/torchsnapshot_amd/ops/hip",
           f"{REPO}/tests/native/mx_codec_selftest.cpp", "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "selftest OK" in run.stdout, run.stdout + run.stderr
