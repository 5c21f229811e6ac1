"""Re-saving onto a committed filesystem path: payload files are
overwritten in place (storage/fs.py) and the old commit is withdrawn first
(Snapshot._uncommit), so the result is the new state or no snapshot at
all, never the old metadata over half-new payloads."""

import errno
import json
import os

import pytest
import torch

import torchsnapshot_amd.snapshot as snapshot_mod
from torchsnapshot_amd import Snapshot, StateDict
from torchsnapshot_amd.storage.fs import FSStoragePlugin
from torchsnapshot_amd.test_utils import tmp_snapshot_path

METADATA = ".snapshot_metadata"


def _big_state() -> StateDict:
    g = torch.Generator().manual_seed(11)
    return StateDict(
        a=torch.rand(1024, 1024, generator=g),  # 4 MiB
        b=torch.rand(300, 1000, generator=g),
        step=1,
    )


def _small_state() -> StateDict:
    # same keys, so the same payload names: "a" shrinks but stays above the
    # 1 MiB in-place threshold (old tail must go), "b" drops below it
    g = torch.Generator().manual_seed(12)
    return StateDict(
        a=torch.rand(600, 1000, generator=g),  # 2.4 MB
        b=torch.rand(10, generator=g),
        step=2,
    )


def _assert_restores(path: str, sd: StateDict) -> None:
    out = StateDict(
        a=torch.zeros_like(sd["a"]), b=torch.zeros_like(sd["b"]), step=0
    )
    Snapshot(path).restore({"sd": out})
    assert torch.equal(out["a"], sd["a"])
    assert torch.equal(out["b"], sd["b"])
    assert out["step"] == sd["step"]


@pytest.mark.parametrize("checksums", [False, True], ids=["plain", "verified"])
def test_resave_smaller_state(toggle_batching, monkeypatch, checksums):
    if checksums:
        monkeypatch.setenv("TSAMD_CHECKSUM", "1")
        monkeypatch.setenv("TSAMD_VERIFY_CHECKSUM", "1")
    first, second = _big_state(), _small_state()
    with tmp_snapshot_path() as path:
        Snapshot.take(path, {"sd": first})
        _assert_restores(path, first)
        Snapshot.take(path, {"sd": second})
        with open(os.path.join(path, METADATA)) as f:
            meta = json.load(f)
        assert meta["manifest"]
        _assert_restores(path, second)


class _FailingFS(FSStoragePlugin):
    """Filesystem plugin whose payload writes fail (metadata and checksum
    files, whose names start with a dot, would still go through)."""

    async def write(self, write_io):
        if not os.path.basename(write_io.path).startswith("."):
            raise OSError(errno.EIO, "injected payload write failure")
        await super().write(write_io)


def test_failed_resave_leaves_path_uncommitted(toggle_batching, monkeypatch):
    first, second = _big_state(), _small_state()
    with tmp_snapshot_path() as path:
        Snapshot.take(path, {"sd": first})
        assert os.path.exists(os.path.join(path, METADATA))

        with monkeypatch.context() as m:
            m.setattr(
                snapshot_mod,
                "url_to_storage_plugin",
                lambda url, opts=None: _FailingFS(url),
            )
            with pytest.raises(OSError, match="injected"):
                Snapshot.take(path, {"sd": second})

        # the old commit is gone: the path reads as "no snapshot here"
        assert not os.path.exists(os.path.join(path, METADATA))
        with pytest.raises((RuntimeError, ValueError)):
            _ = Snapshot(path).metadata

        # and it is reusable
        Snapshot.take(path, {"sd": second})
        _assert_restores(path, second)


def test_first_save_needs_no_existing_metadata():
    # _uncommit on a path that was never committed is a no-op
    with tmp_snapshot_path() as path:
        storage = FSStoragePlugin(path)
        try:
            Snapshot._uncommit(storage)
        finally:
            storage.sync_close()
        sd = _small_state()
        Snapshot.take(path, {"sd": sd})
        _assert_restores(path, sd)
