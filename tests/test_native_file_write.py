"""Payload writer of the filesystem backend: the native one
(``_csnap.file_write``, ops/hip/file_sink.h) and the Python fallback must
put the same bytes on disk under both write policies (overwrite in place /
truncate and rewrite)."""

import errno
import os

import pytest

from torchsnapshot_amd.storage import fs

_csnap = pytest.importorskip(
    "torchsnapshot_amd._csnap", reason="_csnap extension not built"
)

MIB = 1 << 20
CHUNK = 256 * MIB


def _native(path, buf, fsync=False, chunk_bytes=CHUNK, reuse=True):
    return _csnap.file_write(
        path, buf, fsync=fsync, chunk_bytes=chunk_bytes, reuse=reuse
    )


def _python(path, buf, fsync=False, chunk_bytes=CHUNK, reuse=True):
    return fs._write_file_py(path, buf, fsync, chunk_bytes, reuse)


@pytest.fixture(params=[_native, _python], ids=["native", "python"])
def write(request):
    return request.param


def _pattern(n: int, seed: int) -> bytes:
    # position-dependent and seed-dependent, so a stale or shifted byte shows
    block = bytes((i * 7 + seed) & 0xFF for i in range(4099))
    return (block * (n // len(block) + 1))[:n]


def _read(path) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def _nfds() -> int:
    return len(os.listdir("/proc/self/fd"))


def test_fresh_file(tmp_path, write):
    p = str(tmp_path / "payload")
    data = _pattern(3 * MIB + 5, 1)
    assert write(p, data) is False
    assert os.path.getsize(p) == len(data)
    assert _read(p) == data


def test_overwrite_same_size_keeps_inode(tmp_path, write):
    p = str(tmp_path / "payload")
    write(p, _pattern(2 * MIB, 1))
    ino = os.stat(p).st_ino
    new = _pattern(2 * MIB, 2)
    assert write(p, new) is True
    assert os.stat(p).st_ino == ino
    assert _read(p) == new


def test_overwrite_shorter_drops_old_tail(tmp_path, write):
    p = str(tmp_path / "payload")
    write(p, _pattern(2 * MIB, 1))
    new = _pattern(MIB + 13, 2)
    assert write(p, new) is True
    assert os.path.getsize(p) == MIB + 13
    assert _read(p) == new


def test_overwrite_longer(tmp_path, write):
    p = str(tmp_path / "payload")
    write(p, _pattern(MIB + 13, 1))
    new = _pattern(3 * MIB + 1, 2)
    assert write(p, new) is True
    assert os.path.getsize(p) == len(new)
    assert _read(p) == new


def test_small_chunks_loop(tmp_path, write):
    p = str(tmp_path / "payload")
    data = _pattern(MIB + 13, 3)
    write(p, data, chunk_bytes=4096)  # 257 pwrites, the last of 13 bytes
    assert _read(p) == data
    new = _pattern(MIB + 13, 4)
    assert write(p, new, chunk_bytes=4096) is True
    assert _read(p) == new


def test_tiny_payload_over_longer_file(tmp_path, write):
    p = str(tmp_path / "payload")
    write(p, _pattern(2 * MIB, 1))
    new = _pattern(MIB - 1, 2)  # under the reuse threshold: truncate path
    assert write(p, new) is False
    assert os.path.getsize(p) == MIB - 1
    assert _read(p) == new


def test_empty_payload_over_old_file(tmp_path, write):
    p = str(tmp_path / "payload")
    write(p, _pattern(2 * MIB, 1))
    assert write(p, b"") is False
    assert os.path.getsize(p) == 0
    p2 = str(tmp_path / "fresh_empty")
    write(p2, b"")
    assert os.path.getsize(p2) == 0


def test_readonly_bytes_and_offset_memoryview(tmp_path, write):
    p = str(tmp_path / "payload")
    data = _pattern(MIB + 64, 5)  # bytes: a read-only exporter
    write(p, data)
    assert _read(p) == data
    backing = bytearray(_pattern(2 * MIB + 100, 6))
    view = memoryview(backing)[37 : 37 + MIB + 13]
    assert write(p, view) is True
    assert _read(p) == bytes(backing[37 : 37 + MIB + 13])


def test_reuse_false_truncates(tmp_path, write):
    p = str(tmp_path / "payload")
    write(p, _pattern(2 * MIB, 1))
    new = _pattern(MIB + 13, 2)
    assert write(p, new, reuse=False) is False
    assert os.path.getsize(p) == MIB + 13
    assert _read(p) == new


def test_fsync_path(tmp_path, write):
    p = str(tmp_path / "payload")
    data = _pattern(MIB + 13, 7)
    write(p, data, fsync=True)
    assert write(p, data[::-1], fsync=True) is True
    assert _read(p) == data[::-1]


def test_missing_directory_raises_without_leaking_fd(tmp_path, write):
    p = str(tmp_path / "no_such_dir" / "payload")
    before = _nfds()
    for size in (16, 2 * MIB):
        with pytest.raises(OSError) as ei:
            write(p, _pattern(size, 1))
        assert ei.value.errno == errno.ENOENT
        assert ei.value.filename == p
    assert _nfds() == before


def test_unwritable_target_raises_without_leaking_fd(tmp_path, write):
    # a directory can be opened for writing by nobody, root included
    target = tmp_path / "is_a_dir"
    target.mkdir()
    before = _nfds()
    for size in (16, 2 * MIB):
        with pytest.raises(OSError) as ei:
            write(str(target), _pattern(size, 1))
        assert ei.value.errno == errno.EISDIR
        assert ei.value.filename == str(target)
    assert _nfds() == before


def test_write_error_after_open_closes_fd(write):
    # /dev/full opens fine and fails every write with ENOSPC: the error
    # path after a successful open
    if not os.path.exists("/dev/full"):
        pytest.skip("no /dev/full")
    before = _nfds()
    for size in (16, 2 * MIB):
        with pytest.raises(OSError) as ei:
            write("/dev/full", _pattern(size, 1))
        assert ei.value.errno == errno.ENOSPC
    assert _nfds() == before


def test_bad_chunk_bytes(tmp_path, write):
    with pytest.raises(ValueError):
        write(str(tmp_path / "payload"), b"abc", chunk_bytes=0)


def test_plugin_follows_knob(tmp_path, monkeypatch):
    """FSStoragePlugin routes through the writer and honours
    TSAMD_FS_REUSE_PAGES per write."""
    from torchsnapshot_amd.io_types import WriteIO

    plugin = fs.FSStoragePlugin(str(tmp_path))
    try:
        plugin.sync_write(WriteIO("0/slab", _pattern(2 * MIB, 1)))
        full = str(tmp_path / "0" / "slab")
        seen = []
        real = fs.write_file

        def spy(*args, **kwargs):
            seen.append(real(*args, **kwargs))
            return seen[-1]

        monkeypatch.setattr(fs, "write_file", spy)
        new = _pattern(MIB + 13, 2)
        plugin.sync_write(WriteIO("0/slab", new))
        monkeypatch.setenv("TSAMD_FS_REUSE_PAGES", "0")
        plugin.sync_write(WriteIO("0/slab", new))
        # durable saves truncate whatever the knob says
        monkeypatch.setenv("TSAMD_FS_REUSE_PAGES", "1")
        monkeypatch.setenv("TSAMD_FSYNC", "1")
        plugin.sync_write(WriteIO("0/slab", new))
        assert seen == [True, False, False]
        assert _read(full) == new
    finally:
        plugin.sync_close()
