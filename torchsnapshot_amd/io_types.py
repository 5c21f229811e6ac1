"""Core I/O abstractions shared by preparers, scheduler and storage.

Parity with reference torchsnapshot/io_types.py:24-120, re-designed around
an always-off-main-thread asyncio pipeline (see scheduler.py):

- ``BufferStager`` produces the bytes for one write request (for device
  tensors this drives the HIP staging engine: gather-pack kernel + D2H into
  pinned memory).
- ``BufferConsumer`` applies the bytes of one read request to its
  destination (H2D + strided scatter for device tensors).
- ``StoragePlugin`` moves bytes to/from a storage backend, async.
"""

from __future__ import annotations

import abc
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Any, Optional, Tuple

BufferType = Any  # bytes | bytearray | memoryview


@dataclass
class StageContext:
    """Resources available to stagers/consumers during pipeline execution."""

    executor: ThreadPoolExecutor
    # Per-call flag: async snapshots must defensively copy CPU tensors that
    # training might mutate after async_take returns.
    is_async: bool = False


class BufferStager(abc.ABC):
    # "psum64:<hex>" of the staged bytes when staging computed it anyway
    # (the gather kernel does); the write pipeline then skips its own hash
    precomputed_checksum: Optional[str] = None
    # [(start, end, "psum64:<hex>")] per slab member, so byte-range and
    # merged-span reads of the slab can be verified on restore
    member_checksums: Optional[list] = None

    @abc.abstractmethod
    async def stage_buffer(self, ctx: StageContext) -> BufferType:
        """Produce the serialized bytes for this write request."""

    @abc.abstractmethod
    def get_staging_cost_bytes(self) -> int:
        """Peak host-memory cost of staging this buffer (for budgeting)."""

    def release_buffer(self) -> None:
        """Called once the storage write completed; return pooled buffers."""


class BufferConsumer(abc.ABC):
    """Only the two abstract methods are required. The rest is the protocol
    the read scheduler and the span batcher speak to device-bound consumers;
    the defaults describe a consumer that takes host bytes and nothing else."""

    # (psum64 value, word_base) the read scheduler sets before consume_buffer
    # when will_verify_on_device() answered True: the consumer must then
    # check the payload on the device and raise on a mismatch
    expected_psum: Optional[Tuple[int, int]] = None

    @abc.abstractmethod
    async def consume_buffer(self, ctx: StageContext, buf: BufferType) -> None:
        """Apply the read bytes to the destination object."""

    @abc.abstractmethod
    def get_consuming_cost_bytes(self) -> int:
        """Peak host-memory cost of holding + consuming this buffer."""

    def close(self) -> None:
        """Called when the pipeline is done with this request (success or
        failure); return pooled buffers here."""

    def will_verify_on_device(self) -> bool:
        """Asked after the read landed: True when consume_buffer will take
        the bytes to the GPU and can checksum them there, so the scheduler
        hands over ``expected_psum`` instead of hashing on the CPU."""
        return False

    def device_span_target(self) -> Optional[Any]:
        """The device on which this consumer can take its bytes as a slice
        of a device-resident uint8 span (consume_from_device_u8), or None."""
        return None

    def scatter_members(
        self, base_offset: int, verified: bool = False
    ) -> Optional[list]:
        """StagingEngine.scatter members that complete this consumer from a
        pinned read whose byte ``base_offset`` is the payload's first, or
        None when it needs another path. For a ``verified`` (checksummed)
        scatter they must cover the payload exactly once."""
        return None

    def consume_from_device_u8(self, dev_u8: Any) -> None:
        """Apply the payload given as a contiguous device uint8 tensor.
        Required of consumers whose device_span_target() is not None."""
        raise NotImplementedError


@dataclass
class WriteReq:
    path: str
    stager: BufferStager
    # The TensorEntry whose location/byte_range the batcher relocates when
    # this request is packed into a slab (None = not batchable).
    tensor_entry: Optional[Any] = None


@dataclass
class ReadReq:
    path: str
    consumer: BufferConsumer
    byte_range: Optional[Tuple[int, int]] = None
    # Optional allocator for the read buffer (nbytes -> writable
    # memoryview). Device-targeted consumers hand out pinned memory here so
    # storage reads land directly in DMA-able pages (no bounce copy).
    buf_alloc: Optional[Any] = None


@dataclass
class WriteIO:
    path: str
    buf: BufferType


@dataclass
class ReadIO:
    path: str
    byte_range: Optional[Tuple[int, int]] = None
    buf: Optional[BufferType] = field(default=None)
    buf_alloc: Optional[Any] = None


class StoragePlugin(abc.ABC):
    """A storage backend. All methods are coroutines so network backends can
    interleave many transfers on one event loop; the filesystem backend
    delegates to worker threads (GIL-releasing pwrite/pread)."""

    @abc.abstractmethod
    async def write(self, write_io: WriteIO) -> None:
        ...

    @abc.abstractmethod
    async def read(self, read_io: ReadIO) -> None:
        """Fill ``read_io.buf`` with the (byte-ranged) content of the path."""

    @abc.abstractmethod
    async def delete(self, path: str) -> None:
        ...

    async def delete_dir(self, path: str) -> None:
        raise NotImplementedError

    @abc.abstractmethod
    async def close(self) -> None:
        ...

    async def close_for_loop(self) -> None:
        """Release resources tied to the CURRENT event loop (called when a
        pipeline's loop ends). Backends holding per-loop sessions override
        this; default no-op."""

    # -- sync conveniences (run on a private event loop) --------------------

    def sync_write(self, write_io: WriteIO) -> None:
        from .scheduler import run_coro_sync

        run_coro_sync(self.write(write_io))

    def sync_read(self, read_io: ReadIO) -> None:
        from .scheduler import run_coro_sync

        run_coro_sync(self.read(read_io))

    def sync_close(self) -> None:
        from .scheduler import run_coro_sync

        run_coro_sync(self.close())
