"""The read-consumer protocol, the pinned-read lifecycle and the small
helpers under them, all without a GPU."""

import tempfile

import pytest
import torch

from torchsnapshot_amd import integrity
from torchsnapshot_amd.batcher import BatchedBufferConsumer, batch_read_requests
from torchsnapshot_amd.io_preparers.pinned_read import view_payload
from torchsnapshot_amd.io_preparers.sharded_tensor import ShardConsumer
from torchsnapshot_amd.io_preparers.tensor import (
    LoadFuture,
    TensorBufferConsumer,
    TensorIOPreparer,
    _TensorTileConsumer,
    _TiledReadState,
)
from torchsnapshot_amd.io_types import BufferConsumer, BufferStager, ReadReq
from torchsnapshot_amd.manifest import TensorEntry
from torchsnapshot_amd.ops import staging
from torchsnapshot_amd.scheduler import sync_execute_read_reqs
from torchsnapshot_amd.serialization import dtype_to_str
from torchsnapshot_amd.storage.fs import FSStoragePlugin

pytestmark = pytest.mark.timeout(60)


# ---------------------------------------------------------------------------
# a consumer that implements only the abstract methods
# ---------------------------------------------------------------------------


class _BareConsumer(BufferConsumer):
    def __init__(self) -> None:
        self.got = None

    async def consume_buffer(self, ctx, buf) -> None:
        self.got = bytes(buf)

    def get_consuming_cost_bytes(self) -> int:
        return 64


class _BareStager(BufferStager):
    async def stage_buffer(self, ctx):
        return b""

    def get_staging_cost_bytes(self) -> int:
        return 0


def test_protocol_defaults():
    c = _BareConsumer()
    assert c.expected_psum is None
    assert c.will_verify_on_device() is False
    assert c.device_span_target() is None
    assert c.scatter_members(0) is None
    assert c.scatter_members(256, verified=True) is None
    with pytest.raises(NotImplementedError):
        c.consume_from_device_u8(torch.zeros(4, dtype=torch.uint8))
    c.close()
    s = _BareStager()
    assert s.precomputed_checksum is None
    assert s.member_checksums is None


def test_bare_consumer_whole_file_read():
    data = bytes(range(256)) * 3
    with tempfile.TemporaryDirectory() as d:
        storage = FSStoragePlugin(d)
        with open(f"{d}/f", "wb") as f:
            f.write(data)
        bare = _BareConsumer()
        stats = sync_execute_read_reqs(
            [ReadReq(path="f", consumer=bare)],
            storage,
            memory_budget_bytes=1 << 20,
            rank=0,
            checksums={"f": integrity.psum64_hexdigest(data)},
        )
        storage.sync_close()
    assert stats.done_reqs == 1
    assert bare.got == data


def test_bare_consumer_as_span_member():
    torch.manual_seed(31)
    srcs = [torch.randn(17, 3), torch.randn(40)]
    outs = [torch.zeros(17, 3), torch.zeros(40)]
    bare_bytes = bytes(range(200))
    payloads = [
        bytes(srcs[0].reshape(-1).view(torch.uint8).numpy()),
        bare_bytes,
        bytes(srcs[1].reshape(-1).view(torch.uint8).numpy()),
    ]
    file = bytearray()
    ranges = []
    checksums = {}
    for p in payloads:
        off = (len(file) + 255) // 256 * 256
        file.extend(b"\0" * (off - len(file)))
        file.extend(p)
        ranges.append((off, off + len(p)))
        checksums[integrity.member_key("slab", off, off + len(p))] = (
            integrity.psum64_hexdigest(p, word_base=off // 8)
        )
    bare = _BareConsumer()
    reqs = []
    for i, (src, out) in zip((0, 2), zip(srcs, outs)):
        entry = TensorEntry(
            location="slab",
            serializer="buffer",
            dtype=dtype_to_str(torch.float32),
            shape=list(src.shape),
            byte_range=list(ranges[i]),
        )
        reqs.extend(TensorIOPreparer.prepare_read(entry, out)[0])
    reqs.insert(1, ReadReq(path="slab", consumer=bare, byte_range=ranges[1]))
    (span,) = batch_read_requests(reqs)
    assert isinstance(span.consumer, BatchedBufferConsumer)
    assert len(span.consumer.members) == 3
    with tempfile.TemporaryDirectory() as d:
        storage = FSStoragePlugin(d)
        with open(f"{d}/slab", "wb") as f:
            f.write(file)
        stats = sync_execute_read_reqs(
            [span], storage, memory_budget_bytes=1 << 20, rank=0,
            checksums=checksums,
        )
        storage.sync_close()
    assert stats.done_reqs == 1
    assert bare.got == bare_bytes
    for src, out in zip(srcs, outs):
        assert torch.equal(out, src)


# ---------------------------------------------------------------------------
# pinned-read lifecycle
# ---------------------------------------------------------------------------


class _PlainPool(staging.PinnedPool):
    """A pool of ordinary (unpinned) host blocks that counts releases."""

    def __init__(self) -> None:
        super().__init__(block_size=64, block_count=2)
        self.released = 0

    def _alloc(self, nbytes: int) -> torch.Tensor:
        return torch.empty(nbytes, dtype=torch.uint8)

    def release(self, block) -> None:
        self.released += 1
        super().release(block)


def _entry():
    return TensorEntry(
        location="t", serializer="buffer", dtype=dtype_to_str(torch.float32), shape=[2]
    )


def _make_tensor_consumer():
    return TensorBufferConsumer(_entry(), None, LoadFuture())


def _make_shard_consumer():
    return ShardConsumer(shard_entry=_entry(), targets=[])


def _make_span_consumer():
    return BatchedBufferConsumer(members=[], span_start=0)


def _make_tile_consumer():
    staging_t = torch.zeros(8, dtype=torch.uint8)
    state = _TiledReadState(remaining=1, staging=staging_t, tensor_out=None)
    return _TensorTileConsumer(dst_flat_u8=staging_t, start=0, end=8, state=state)


@pytest.fixture
def plain_pool(monkeypatch):
    pool = _PlainPool()
    monkeypatch.setattr(staging, "_pool", pool)
    return pool


@pytest.mark.parametrize("nbytes", [0, 1, 100], ids=["n0", "n1", "oversized"])
@pytest.mark.parametrize(
    "make",
    [
        _make_tensor_consumer,
        _make_shard_consumer,
        _make_span_consumer,
        _make_tile_consumer,
    ],
    ids=["tensor", "shard", "span", "tile"],
)
def test_pinned_lifecycle(make, nbytes, plain_pool):
    consumer = make()
    consumer.close()  # nothing allocated: nothing to release
    assert plain_pool.released == 0

    view = consumer.alloc_pinned_buffer(nbytes)
    assert isinstance(view, memoryview)
    assert view.nbytes == nbytes and not view.readonly
    if nbytes:
        view[:] = bytes([7]) * nbytes
        assert bytes(view) == bytes([7]) * nbytes
    consumer.close()
    assert plain_pool.released == 1
    # a pooled block is back on the free list, a one-off never joins it
    assert len(plain_pool._free) == (1 if nbytes <= plain_pool.block_size else 0)
    consumer.close()
    assert plain_pool.released == 1
    assert len(plain_pool._free) <= 1


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("value", [0, 1, 2**64 - 1])
def test_psum64_format_parse_round_trip(value):
    text = integrity.format_psum64(value)
    assert text == "psum64:" + format(value, "016x")
    assert integrity.parse_psum64(text) == value


def test_psum64_format_matches_hexdigest_and_parser_rejects_others():
    assert integrity.format_psum64(0) == integrity.psum64_hexdigest(b"")
    assert integrity.parse_psum64("xxh3:0123456789abcdef") is None
    assert integrity.parse_psum64("0123456789abcdef") is None
    assert integrity.parse_psum64("") is None
    assert integrity.parse_psum64(None) is None


def test_view_payload():
    u8 = torch.arange(12, dtype=torch.uint8)
    same = view_payload(u8, torch.uint8, (3, 4))
    assert same.dtype == torch.uint8 and same.shape == (3, 4)
    assert torch.equal(same.reshape(-1), u8)

    bf = torch.randn(2, 3).to(torch.bfloat16)
    got = view_payload(bf.reshape(-1).view(torch.uint8), torch.bfloat16, [2, 3])
    assert got.dtype == torch.bfloat16 and torch.equal(got, bf)

    empty = view_payload(torch.empty(0, dtype=torch.uint8), torch.float32, (0, 7))
    assert empty.dtype == torch.float32 and empty.shape == (0, 7)

    scalar = torch.tensor(2.5)
    got = view_payload(scalar.reshape(1).view(torch.uint8), torch.float32, ())
    assert got.shape == () and got.item() == 2.5
