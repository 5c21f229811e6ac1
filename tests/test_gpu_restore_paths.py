"""GPU tests: the device-restore paths a read takes when the scatter kernel
is not in play.

1. No pinned block: the storage layer handed back plain bytes (an object
   store, or a member of a span that is not all-device), so the payload is
   bounced through the pinned pool.
2. A slab whose members go to cpu and cuda targets alternately.
3. A tiled read straight into a device tensor.

Every test runs under each TSAMD_RESTORE_MODE, and the oracle is the source
tensor itself (bit equality) or the CPU psum64 of the same bytes."""

import asyncio
import glob
import os
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from torchsnapshot_amd import Snapshot, StateDict, integrity  # noqa: E402
from torchsnapshot_amd.batcher import (  # noqa: E402
    BatchedBufferConsumer,
    batch_read_requests,
)
from torchsnapshot_amd.io_preparers.sharded_tensor import (  # noqa: E402
    plan_shard_reads,
)
from torchsnapshot_amd.io_preparers.tensor import TensorIOPreparer  # noqa: E402
from torchsnapshot_amd.io_types import StageContext  # noqa: E402
from torchsnapshot_amd.manifest import Shard, TensorEntry  # noqa: E402
from torchsnapshot_amd.ops import staging  # noqa: E402
from torchsnapshot_amd.serialization import dtype_to_str  # noqa: E402
from torchsnapshot_amd.test_utils import tmp_snapshot_path  # noqa: E402


@pytest.fixture(params=["torch", "direct", "slab"], autouse=True)
def restore_mode(request, monkeypatch):
    monkeypatch.setenv("TSAMD_RESTORE_MODE", request.param)
    return request.param


@pytest.fixture
def scatter_calls(monkeypatch):
    calls = []
    orig = staging.StagingEngine.scatter

    def wrapped(self, pinned_block, nbytes, members, *args, **kwargs):
        calls.append(len(members))
        return orig(self, pinned_block, nbytes, members, *args, **kwargs)

    monkeypatch.setattr(staging.StagingEngine, "scatter", wrapped)
    return calls


def _bytes_of(t: torch.Tensor) -> bytes:
    c = t.detach().cpu().contiguous().reshape(-1)
    return bytes(c.view(torch.uint8).numpy()) if c.numel() else b""


def _feed_plain(read_reqs, payload_of):
    """What the read pipeline does when the storage layer ignores
    buf_alloc: consume_buffer gets a plain bytes object."""

    async def run():
        with ThreadPoolExecutor(max_workers=2) as ex:
            ctx = StageContext(executor=ex)
            for req in read_reqs:
                try:
                    await req.consumer.consume_buffer(ctx, payload_of[req.path])
                finally:
                    req.consumer.close()

    asyncio.run(run())


def _flip_byte(path: str, pos: int) -> None:
    with open(path, "r+b") as f:
        f.seek(pos)
        b = f.read(1)
        f.seek(pos)
        f.write(bytes([b[0] ^ 0x40]))


def _payload_files(root: str):
    return [
        p
        for p in glob.glob(os.path.join(root, "**"), recursive=True)
        if os.path.isfile(p)
        and not p.endswith((".snapshot_metadata", ".checksums"))
    ]


# ---------------------------------------------------------------------------
# 1. no pinned block
# ---------------------------------------------------------------------------


def _tensor_cases():
    torch.manual_seed(21)
    f32 = torch.randn(129, 33)
    bf16 = torch.randn(129, 33).to(torch.bfloat16)
    u8 = torch.randint(0, 256, (7, 5), dtype=torch.uint8)
    return {
        "f32_transposed": (f32, lambda: torch.zeros(33, 129, device="cuda").t()),
        "bf16_into_f32": (bf16, lambda: torch.zeros(129, 33, device="cuda")),
        "u8": (u8, lambda: torch.zeros(7, 5, dtype=torch.uint8, device="cuda")),
    }


@pytest.mark.parametrize("case", ["f32_transposed", "bf16_into_f32", "u8"])
def test_tensor_consumer_without_pinned_block(case, scatter_calls):
    """No zero-element case here: an empty payload handed over as plain
    bytes reaches ``torch.frombuffer`` in the bounce step, which refuses a
    zero-length buffer with ValueError. That is how the bounce step has
    always behaved (an empty tensor read into a pinned block is fine)."""
    src, make_out = _tensor_cases()[case]
    out = make_out()
    entry = TensorEntry(
        location="t",
        serializer="buffer",
        dtype=dtype_to_str(src.dtype),
        shape=list(src.shape),
    )
    reqs, fut = TensorIOPreparer.prepare_read(entry, out)
    _feed_plain(reqs, {"t": _bytes_of(src)})
    assert scatter_calls == []
    assert fut.obj is out
    assert torch.equal(out.cpu(), src.to(out.dtype))


def _span_fixture():
    """Three members of one file at 256-aligned byte ranges, all-cuda
    targets, merged into one span read."""
    torch.manual_seed(22)
    srcs = [torch.randn(199, 33), torch.randn(64, 64), torch.randn(5)]
    outs = [torch.zeros(s.shape, device="cuda") for s in srcs]
    file = bytearray()
    off = 512  # the span starts inside the file: a non-zero word base
    reqs = []
    for src, out in zip(srcs, outs):
        data = _bytes_of(src)
        file.extend(b"\0" * (off - len(file)))
        file.extend(data)
        entry = TensorEntry(
            location="slab",
            serializer="buffer",
            dtype=dtype_to_str(torch.float32),
            shape=list(src.shape),
            byte_range=[off, off + len(data)],
        )
        reqs.extend(TensorIOPreparer.prepare_read(entry, out)[0])
        off = (off + len(data) + 255) // 256 * 256
    (span,) = batch_read_requests(reqs)
    assert isinstance(span.consumer, BatchedBufferConsumer)
    start, end = span.byte_range
    assert start == 512 and start % 256 == 0
    return span, bytes(file[start:end]), srcs, outs


@pytest.mark.parametrize("psum", ["unset", "right", "wrong"])
def test_span_consumer_without_pinned_block(psum, scatter_calls):
    span, span_bytes, srcs, outs = _span_fixture()
    word_base = span.byte_range[0] // 8
    value = integrity.psum64_value(span_bytes, word_base)
    if psum == "right":
        span.consumer.expected_psum = (value, word_base)
    elif psum == "wrong":
        span.consumer.expected_psum = ((value + 1) % (1 << 64), word_base)
    if psum == "wrong":
        with pytest.raises(RuntimeError, match="checksum mismatch"):
            _feed_plain([span], {"slab": span_bytes})
    else:
        _feed_plain([span], {"slab": span_bytes})
        for src, out in zip(srcs, outs):
            assert torch.equal(out.cpu(), src)
    assert scatter_calls == []


@pytest.mark.parametrize("stored", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("split", ["rows", "cols"])
def test_shard_consumer_without_pinned_block(split, stored, scatter_calls):
    """The 90 x 66, 2-to-3 layout of test_reshard_2_to_3."""
    torch.manual_seed(23)
    rows, cols = 90, 66
    full = torch.randn(rows, cols).to(stored)
    dim = 0 if split == "rows" else 1
    n = full.shape[dim]
    shards, payload_of = [], {}
    for i, (off, ln) in enumerate([(0, n // 2), (n // 2, n - n // 2)]):
        piece = full.narrow(dim, off, ln)
        offsets = [0, 0]
        offsets[dim] = off
        entry = TensorEntry(
            location=f"shard{i}",
            serializer="buffer",
            dtype=dtype_to_str(stored),
            shape=list(piece.shape),
        )
        shards.append(Shard(offsets=offsets, sizes=list(piece.shape), tensor=entry))
        payload_of[entry.location] = _bytes_of(piece)
    out = torch.zeros(rows, cols, device="cuda")  # f32: bf16 shards widen
    targets = []
    for off, ln in [(0, n // 3), (n // 3, n // 3), (2 * (n // 3), n - 2 * (n // 3))]:
        offsets = [0, 0]
        offsets[dim] = off
        targets.append((out.narrow(dim, off, ln), offsets))
    reqs = plan_shard_reads(shards, targets)
    assert len(reqs) == 2
    _feed_plain(reqs, payload_of)
    assert scatter_calls == []
    assert torch.equal(out.cpu(), full.to(torch.float32))


# ---------------------------------------------------------------------------
# 2. mixed span
# ---------------------------------------------------------------------------


def test_mixed_cpu_cuda_span_verifies(monkeypatch):
    monkeypatch.setenv("TSAMD_CHECKSUM", "1")
    monkeypatch.setenv("TSAMD_SLAB_SIZE_THRESHOLD_BYTES", str(1024 * 1024))
    torch.manual_seed(24)
    shapes = [(37, 5), (64,), (3, 3, 3), (129,), (2, 50), (1,)]
    src = StateDict(
        **{f"t{i}": torch.randn(*s, device="cuda") for i, s in enumerate(shapes)}
    )

    def zeros():
        return StateDict(
            **{
                f"t{i}": torch.zeros(*s, device="cuda" if i % 2 else "cpu")
                for i, s in enumerate(shapes)
            }
        )

    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": src})
        (slab,) = _payload_files(path)  # all six in one slab
        monkeypatch.setenv("TSAMD_VERIFY_CHECKSUM", "1")
        out = zeros()
        snap.restore({"sd": out})
        for i, k in enumerate(src):
            assert out[k].device.type == ("cuda" if i % 2 else "cpu")
            assert torch.equal(out[k].cpu(), src[k].cpu()), k
        _flip_byte(slab, 64)
        with pytest.raises(RuntimeError, match="checksum mismatch"):
            snap.restore({"sd": zeros()})
        _flip_byte(slab, 64)
        snap.restore({"sd": zeros()})


# ---------------------------------------------------------------------------
# 3. tiled read into a device tensor
# ---------------------------------------------------------------------------


def test_tiled_read_into_device_tensor(monkeypatch):
    monkeypatch.setenv("TSAMD_CHECKSUM", "1")
    torch.manual_seed(25)
    src = torch.randn(160, 64, device="cuda")
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": StateDict(w=src)})
        monkeypatch.setenv("TSAMD_VERIFY_CHECKSUM", "1")
        out = torch.zeros(160, 64, device="cuda")
        got = snap.read_object("0/sd/w", obj_out=out, memory_budget_bytes=4096)
        assert got is out
        assert torch.equal(out, src)
        (payload,) = _payload_files(path)
        _flip_byte(payload, 4096 + 64)  # inside the second tile
        with pytest.raises(RuntimeError, match="checksum mismatch"):
            snap.read_object(
                "0/sd/w",
                obj_out=torch.zeros(160, 64, device="cuda"),
                memory_budget_bytes=4096,
            )
