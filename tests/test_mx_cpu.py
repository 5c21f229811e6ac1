"""Block-scaled fp8 saves on the host: mx_encode / mx_decode against the
float64 reference of docs/format.md, and save_dtype="mxfp8_e4m3" through
take and restore."""

import os

import pytest
import torch

import torchsnapshot_amd
from torchsnapshot_amd import Snapshot, StateDict
from torchsnapshot_amd.io_preparers.chunked_tensor import ChunkedTensorIOPreparer
from torchsnapshot_amd.manifest import ChunkedTensorEntry
from torchsnapshot_amd.manifest_ops import _merge_replicated_entries
from torchsnapshot_amd.ops.staging import mx_decode, mx_encode
from torchsnapshot_amd.test_utils import run_multiprocess

from _mx_reference import assert_error_bound, decoded_as, edge_values, mx_reference

MX = "mxfp8_e4m3"
DTYPES = [torch.float32, torch.bfloat16]
SAME = dict(rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 33 * 65])
def test_encode_decode_match_reference(n, dtype):
    t = edge_values(n, dtype)
    if n == 33 * 65:  # a transposed view: blocks follow the logical order
        t = t.reshape(65, 33).t()
    payload, decoded, E = mx_reference(t)
    assert_error_bound(t, decoded, E)
    got = mx_encode(t)
    assert got.dtype == torch.uint8 and got.numel() == 33 * (-(-n // 32))
    assert torch.equal(got, payload)
    for target in DTYPES:
        got = mx_decode(payload, n, target)
        torch.testing.assert_close(got, decoded_as(decoded, target), **SAME)


@pytest.mark.parametrize("batching", ["0", "1"])
def test_take_restore_roundtrip(tmp_path, monkeypatch, batching):
    monkeypatch.setenv("TSAMD_DISABLE_BATCHING", batching)
    src = StateDict(
        w=edge_values(700, torch.float32).reshape(7, 100),
        b=edge_values(300, torch.bfloat16),
        i=torch.arange(10),
    )
    assert torchsnapshot_amd.MXFP8_E4M3 == MX
    snap = Snapshot.take(str(tmp_path / "s"), {"m": src}, save_dtype=MX)
    manifest = snap.get_manifest()
    for name, logical in (("w", "float32"), ("b", "bfloat16")):
        entry = manifest[f"0/m/{name}"]
        assert entry["dtype"] == MX and entry["logical_dtype"] == logical
    out = StateDict(
        w=torch.zeros(7, 100, dtype=torch.float64),
        b=torch.zeros(300, dtype=torch.bfloat16),
        i=torch.zeros(10, dtype=torch.long),
    )
    snap.restore({"m": out})
    want_w = decoded_as(mx_reference(src["w"])[1], torch.float32).reshape(7, 100)
    want_b = decoded_as(mx_reference(src["b"])[1], torch.bfloat16)
    torch.testing.assert_close(out["w"], want_w.double(), **SAME)
    torch.testing.assert_close(out["b"], want_b, **SAME)
    assert torch.equal(out["i"], src["i"])
    torch.testing.assert_close(snap.read_object("0/m/b"), want_b, **SAME)
    diff = snap.compare({"m": src})
    assert diff["m/w"].note is not None and diff["m/i"].n_diff == 0


def test_chunked_leaf_blocks_start_at_each_chunk(tmp_path, monkeypatch):
    monkeypatch.setenv("TSAMD_MAX_CHUNK_SIZE_BYTES", str(40 * 4 * 3))
    t = edge_values(7 * 40, torch.float32).reshape(7, 40)
    snap = Snapshot.take(str(tmp_path / "s"), {"m": StateDict(t=t)}, save_dtype=MX)
    entry = snap.get_manifest()["0/m/t"]
    assert entry["kind"] == "chunked_tensor" and entry["logical_dtype"] == "float32"
    out = StateDict(t=torch.zeros(7, 40))
    snap.restore({"m": out})
    parts = [mx_reference(t[lo : lo + 3])[1] for lo in (0, 3, 6)]
    want = decoded_as(torch.cat(parts), torch.float32).reshape(7, 40)
    torch.testing.assert_close(out["t"], want, **SAME)
    # a replicated leaf's chunks, written by several ranks, merge on load
    halves = [ChunkedTensorEntry.from_dict({**entry, "chunks": c}) for c in
              (entry["chunks"][:2], entry["chunks"][2:])]
    merged = _merge_replicated_entries(halves)
    assert merged.logical_dtype == "float32" and len(merged.chunks) == 3
    assert ChunkedTensorIOPreparer.prepare_read(merged)[1].obj.dtype == torch.float32


def _sharded_left_as_is(tmpdir: str) -> None:
    from torch.distributed._shard import sharded_tensor
    from torch.distributed._shard.sharding_spec import ChunkShardingSpec

    st = sharded_tensor.rand(ChunkShardingSpec(dim=0, placements=["rank:0/cpu"]), (48, 8))
    snap = Snapshot.take(
        os.path.join(tmpdir, "s"), {"m": StateDict(st=st)}, save_dtype=MX
    )
    entry = snap.get_manifest()["0/m/st"]
    assert entry["dtype"] == "float32"
    assert all(s["tensor"]["dtype"] == "float32" for s in entry["shards"])


def test_sharded_leaf_is_left_unnarrowed(tmp_path):
    run_multiprocess(1, _sharded_left_as_is, str(tmp_path))
