"""Reads that land in pinned memory, and the one ladder that takes a payload
bound for device tensors from there (or from a plain buffer) to the GPU."""

from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from ..io_types import BufferConsumer, BufferType
from ..ops.staging import get_pinned_pool, get_staging_engine, verify_device_psum


class PinnedReadConsumer(BufferConsumer):
    """A consumer that can offer ``alloc_pinned_buffer`` as its request's
    ReadReq.buf_alloc: the storage layer then reads straight into a block of
    the pinned pool, so H2D needs no bounce copy. A merged span read and
    storage plugins that ignore buf_alloc leave ``_pinned_block`` None."""

    _pinned_block = None
    _pinned_nbytes = 0

    def alloc_pinned_buffer(self, nbytes: int) -> memoryview:
        self._pinned_block = get_pinned_pool().acquire(max(nbytes, 1))
        self._pinned_nbytes = nbytes
        return memoryview(self._pinned_block.tensor.numpy())[:nbytes]

    def close(self) -> None:
        # a block that does not go back starves every later restore
        block, self._pinned_block = self._pinned_block, None
        if block is not None:
            get_pinned_pool().release(block)


def view_payload(
    u8: torch.Tensor, dtype: torch.dtype, shape: Sequence[int]
) -> torch.Tensor:
    """Contiguous uint8 payload bytes as a ``dtype`` tensor of ``shape``."""
    return (u8 if dtype == torch.uint8 else u8.view(dtype)).reshape(tuple(shape))


def payload_to_device(
    consumer: PinnedReadConsumer,
    buf: BufferType,
    device: torch.device,
    members: Optional[Sequence[Tuple[torch.Tensor, torch.dtype, int]]],
    expected_psum: Optional[Tuple[int, int]],
    what: str,
) -> Optional[torch.Tensor]:
    """The restore ladder of a payload whose targets are on ``device``.

    (a) The read landed in the consumer's pinned block and ``members`` names
        scatter targets: ONE StagingEngine.scatter launch straight out of the
        block (widening and the checksum fused in) completes the restore.
        Returns None.
    (b) Pinned block, no members: straight SDMA H2D of the block.
    (c) No pinned block: ``buf`` is bounced through a pool block first (a
        pageable ``.to(device)`` measures ~3x slower on MI355X).

    (b) and (c) return the payload as a device uint8 tensor, checked against
    ``expected_psum`` when that is set, for the caller to view and copy."""
    block, n = consumer._pinned_block, consumer._pinned_nbytes
    bounce = block is None
    if bounce:
        mv = memoryview(buf)
        n = mv.nbytes
        block = get_pinned_pool().acquire(max(n, 1))
    try:
        if bounce:
            block.tensor[:n].copy_(torch.frombuffer(mv, dtype=torch.uint8))
        elif members is not None:
            get_staging_engine(device).scatter(
                block, n, members, expected_psum=expected_psum, what=what
            )
            return None
        dev_u8 = block.tensor[:n].to(device, non_blocking=False)
    finally:
        if bounce:
            get_pinned_pool().release(block)
    if expected_psum is not None:
        verify_device_psum(dev_u8, expected_psum, what)
    return dev_u8
