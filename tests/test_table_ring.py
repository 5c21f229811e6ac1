"""Host-only run of the launch-table ring's slot policy: ops/hip/table_ring.h
is plain C++ with completion as a callback, so a stand-alone program
(tests/native/table_ring_selftest.cpp) is compiled with ASan + UBSan by the
host compiler and run directly. It fills the ring, wraps with the oldest
slot still busy (the wait callback must run first), asks for a table larger
than a slot (no slot, the caller's fallback), a zero-length table, a failing
launch, and eight concurrent launchers. Nothing is loaded into Python under
a sanitizer."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "table_ring_selftest.cpp")
INCLUDE = os.path.join(REPO, "torchsnapshot_amd", "ops", "hip")


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_table_ring_under_asan_ubsan(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "table_ring_selftest")
    build = subprocess.run(
        [
            cxx,
            "-std=c++17",
            "-O1",
            "-g",
            "-fno-omit-frame-pointer",
            "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all",
            "-pthread",
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
    assert "table_ring selftest OK" in run.stdout


def test_ring_constants_exported():
    """The extension reports the ring it was built with."""
    from torchsnapshot_amd.ops import staging

    if not staging.HIP_EXT_AVAILABLE:
        pytest.skip("_csnap not built")
    assert staging._csnap.table_ring_slots() >= 2
    # at least the flagship's slabs: tens of 120-byte descriptor rows
    assert staging._csnap.table_ring_slot_bytes() >= 8 * 1024
