"""Block-scaled fp4 saves on the host: mx4_encode / mx4_decode against the
float64 reference of docs/format.md, and save_dtype="mxfp4_e2m1" through
take and restore."""

import pytest
import torch

import torchsnapshot_amd
from torchsnapshot_amd import Snapshot, StateDict
from torchsnapshot_amd.ops.staging import mx4_decode, mx4_encode

from _mx4_reference import assert_error_bound, edge_values4, mx4_reference
from _mx_reference import decoded_as

MX4 = "mxfp4_e2m1"
DTYPES = [torch.float32, torch.bfloat16]
SAME = dict(rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 33 * 65])
def test_encode_decode_match_reference(n, dtype):
    t = edge_values4(n, dtype)
    if n == 33 * 65:  # a transposed view: blocks follow the logical order
        t = t.reshape(65, 33).t()
    payload, decoded, E = mx4_reference(t)
    assert_error_bound(t, decoded, E)
    got = mx4_encode(t)
    assert got.dtype == torch.uint8 and got.numel() == 17 * (-(-n // 32))
    assert torch.equal(got, payload)
    for target in DTYPES:
        got = mx4_decode(payload, n, target)
        torch.testing.assert_close(got, decoded_as(decoded, target), **SAME)


@pytest.mark.parametrize("batching", ["0", "1"])
def test_take_restore_roundtrip(tmp_path, monkeypatch, batching):
    monkeypatch.setenv("TSAMD_DISABLE_BATCHING", batching)
    src = StateDict(
        w=edge_values4(700, torch.float32).reshape(7, 100),
        b=edge_values4(300, torch.bfloat16),
        i=torch.arange(10),
    )
    assert torchsnapshot_amd.MXFP4_E2M1 == MX4
    snap = Snapshot.take(str(tmp_path / "s"), {"m": src}, save_dtype={"**": MX4})
    manifest = snap.get_manifest()
    for name, logical in (("w", "float32"), ("b", "bfloat16")):
        entry = manifest[f"0/m/{name}"]
        assert entry["dtype"] == MX4 and entry["logical_dtype"] == logical
    out = StateDict(
        w=torch.zeros(7, 100, dtype=torch.float64),
        b=torch.zeros(300, dtype=torch.bfloat16),
        i=torch.zeros(10, dtype=torch.long),
    )
    snap.restore({"m": out})
    want_w = decoded_as(mx4_reference(src["w"])[1], torch.float32).reshape(7, 100)
    want_b = decoded_as(mx4_reference(src["b"])[1], torch.bfloat16)
    torch.testing.assert_close(out["w"], want_w.double(), **SAME)
    torch.testing.assert_close(out["b"], want_b, **SAME)
    assert torch.equal(out["i"], src["i"])
    torch.testing.assert_close(snap.read_object("0/m/b"), want_b, **SAME)
    diff = snap.compare({"m": src})
    assert diff["m/w"].note is not None and diff["m/i"].n_diff == 0


def test_chunked_leaf_blocks_start_at_each_chunk(tmp_path, monkeypatch):
    monkeypatch.setenv("TSAMD_MAX_CHUNK_SIZE_BYTES", str(40 * 4 * 3))
    t = edge_values4(7 * 40, torch.float32).reshape(7, 40)
    snap = Snapshot.take(str(tmp_path / "s"), {"m": StateDict(t=t)}, save_dtype=MX4)
    entry = snap.get_manifest()["0/m/t"]
    assert entry["kind"] == "chunked_tensor" and entry["dtype"] == MX4
    assert entry["logical_dtype"] == "float32"
    out = StateDict(t=torch.zeros(7, 40))
    snap.restore({"m": out})
    parts = [mx4_reference(t[lo : lo + 3])[1] for lo in (0, 3, 6)]
    want = decoded_as(torch.cat(parts), torch.float32).reshape(7, 40)
    torch.testing.assert_close(out["t"], want, **SAME)
