"""ShardedTensor preparer + the resharding overlap machinery.

Write: each rank persists its local shards (subdivided to the max shard
size so staging/storage pipeline). Read (the resharding core): the target
tensor's local shards are intersected with the persisted shards; each
persisted shard is read once and scattered into every overlapping local
view. Restoring works at any world size / sharding spec, or into a plain
full tensor. Parity with reference torchsnapshot/io_preparers/
sharded_tensor.py:48-333.
"""

from __future__ import annotations

import asyncio
import logging
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence, Tuple

import torch

from .. import knobs
from ..io_types import (
    BufferType,
    ReadReq,
    StageContext,
    WriteReq,
)
from ..manifest import Shard as ShardMeta
from ..manifest import ShardedTensorEntry, TensorEntry
from ..ops.staging import HIP_EXT_AVAILABLE, scatter_member
from ..serialization import (
    SERIALIZER_BUFFER,
    dtype_to_str,
    str_to_dtype,
    tensor_from_memoryview,
    torch_load_from_bytes,
)
from .pinned_read import PinnedReadConsumer, payload_to_device, view_payload
from .tensor import LoadFuture, TensorIOPreparer, tensor_copy

logger = logging.getLogger(__name__)


# ---------------------------------------------------------------------------
# overlap machinery (shared with the DTensor preparer)
# ---------------------------------------------------------------------------


@dataclass
class Overlap:
    """Intersection of a persisted shard and a target view, in both frames."""

    src_offsets: List[int]  # within the persisted shard
    dst_offsets: List[int]  # within the target view
    lengths: List[int]


def compute_overlap(
    src_offsets: Sequence[int],
    src_sizes: Sequence[int],
    dst_offsets: Sequence[int],
    dst_sizes: Sequence[int],
) -> Optional[Overlap]:
    so, do, ln = [], [], []
    for s_off, s_sz, d_off, d_sz in zip(
        src_offsets, src_sizes, dst_offsets, dst_sizes
    ):
        lo = max(s_off, d_off)
        hi = min(s_off + s_sz, d_off + d_sz)
        if hi <= lo:
            return None
        so.append(lo - s_off)
        do.append(lo - d_off)
        ln.append(hi - lo)
    return Overlap(src_offsets=so, dst_offsets=do, lengths=ln)


def narrow_nd(
    tensor: torch.Tensor, offsets: Sequence[int], lengths: Sequence[int]
) -> torch.Tensor:
    view = tensor
    for dim, (off, ln) in enumerate(zip(offsets, lengths)):
        view = view.narrow(dim, off, ln)
    return view


def contiguous_source_offset(
    shard_shape: Sequence[int], overlap: "Overlap"
) -> Optional[int]:
    """Element offset of the overlap's source box within the stored shard
    when the box is one contiguous run of it (same-sharding restores, dim-0
    resharding), else None (a general N-d sub-box). Asked of a meta tensor,
    so the answer is torch's own notion of contiguity."""
    box = narrow_nd(
        torch.empty(tuple(shard_shape), device="meta"),
        overlap.src_offsets,
        overlap.lengths,
    )
    return box.storage_offset() if box.is_contiguous() else None


def subdivide_shard(
    tensor: torch.Tensor,
    global_offsets: Sequence[int],
    max_bytes: int,
) -> List[Tuple[torch.Tensor, List[int]]]:
    """Split a local shard along its largest dim into pieces of at most
    ``max_bytes``; returns [(piece, piece_global_offsets), ...]."""
    nbytes = tensor.numel() * tensor.element_size()
    if nbytes <= max_bytes or tensor.dim() == 0:
        return [(tensor, list(global_offsets))]
    dim = max(range(tensor.dim()), key=lambda d: tensor.shape[d])
    if tensor.shape[dim] <= 1:
        return [(tensor, list(global_offsets))]
    row_bytes = max(nbytes // tensor.shape[dim], 1)
    rows_per = max(max_bytes // row_bytes, 1)
    out: List[Tuple[torch.Tensor, List[int]]] = []
    off = 0
    while off < tensor.shape[dim]:
        ln = min(rows_per, tensor.shape[dim] - off)
        piece = tensor.narrow(dim, off, ln)
        piece_offsets = list(global_offsets)
        piece_offsets[dim] += off
        out.append((piece, piece_offsets))
        off += ln
    return out


def location_for_shard(storage_path: str, offsets: Sequence[int]) -> str:
    return f"{storage_path}.{'_'.join(str(o) for o in offsets)}"


# ---------------------------------------------------------------------------
# consumers
# ---------------------------------------------------------------------------


class ShardConsumer(PinnedReadConsumer):
    """Deserialize one persisted shard and scatter it into every
    overlapping target view."""

    def __init__(
        self,
        shard_entry: TensorEntry,
        targets: List[Tuple[torch.Tensor, Overlap]],
    ) -> None:
        self.shard_entry = shard_entry
        self.targets = targets

    def all_targets_on_device(self) -> bool:
        return bool(self.targets) and all(
            dst.device.type == "cuda" for dst, _ in self.targets
        )

    def get_consuming_cost_bytes(self) -> int:
        return self.shard_entry.nbytes_estimate()

    def device_span_target(self):
        if (
            self.all_targets_on_device()
            and self.shard_entry.serializer != "torch_save"
        ):
            return self.targets[0][0].device
        return None

    def will_verify_on_device(self) -> bool:
        # only the pinned -> device path checksums on the GPU
        return (
            HIP_EXT_AVAILABLE
            and self._pinned_block is not None
            and self.device_span_target() is not None
        )

    def scatter_members(self, base_offset: int, verified: bool = False):
        """Every overlap's source box has to be a contiguous run of the
        stored shard, every target eligible and on one device. A
        ``verified`` (checksummed) scatter hashes only what it scatters, so
        the members must then cover the shard's bytes exactly once."""
        if self.shard_entry.serializer != SERIALIZER_BUFFER or not self.targets:
            return None
        stored = str_to_dtype(self.shard_entry.dtype)
        device = self.targets[0][0].device
        members = []
        for dst_view, ov in self.targets:
            src_off = contiguous_source_offset(self.shard_entry.shape, ov)
            if src_off is None or dst_view.device != device:
                return None
            dst = narrow_nd(dst_view.detach(), ov.dst_offsets, ov.lengths)
            member = scatter_member(
                dst, stored, base_offset + src_off * stored.itemsize
            )
            if member is None:
                return None
            members.append(member)
        if verified:
            pos = base_offset
            for dst, _, off in sorted(members, key=lambda m: m[2]):
                if off != pos:
                    return None
                pos += dst.numel() * stored.itemsize
            if pos - base_offset != self.shard_entry.nbytes_estimate():
                return None
        return members

    def consume_from_device_u8(self, dev_u8: torch.Tensor) -> None:
        self._copy_overlaps(
            view_payload(
                dev_u8, str_to_dtype(self.shard_entry.dtype), self.shard_entry.shape
            )
        )

    def _copy_overlaps(self, shard: torch.Tensor) -> None:
        for dst_view, ov in self.targets:
            src = narrow_nd(shard, ov.src_offsets, ov.lengths)
            dst = narrow_nd(dst_view, ov.dst_offsets, ov.lengths)
            tensor_copy(dst, src)

    async def consume_buffer(self, ctx: StageContext, buf: BufferType) -> None:
        def work() -> None:
            if self.shard_entry.serializer == "torch_save":
                shard = torch_load_from_bytes(bytes(buf))
            elif self.all_targets_on_device():
                verified = self.expected_psum is not None
                dev_u8 = payload_to_device(
                    self,
                    buf,
                    self.targets[0][0].device,
                    self.scatter_members(0, verified)
                    if self._pinned_block is not None
                    else None,
                    self.expected_psum,
                    self.shard_entry.location,
                )
                if dev_u8 is not None:  # else the scatter kernel did it all
                    self.consume_from_device_u8(dev_u8)
                return
            else:
                shard = tensor_from_memoryview(
                    memoryview(buf),
                    dtype=str_to_dtype(self.shard_entry.dtype),
                    shape=tuple(self.shard_entry.shape),
                )
            self._copy_overlaps(shard)

        await asyncio.get_running_loop().run_in_executor(ctx.executor, work)


def plan_shard_reads(
    shards: List[ShardMeta],
    targets: List[Tuple[torch.Tensor, Sequence[int]]],
) -> List[ReadReq]:
    """For each persisted shard overlapping any target view, emit one read.

    ``targets``: [(local_view_tensor, view_global_offsets), ...]
    """
    read_reqs: List[ReadReq] = []
    for shard in shards:
        hits: List[Tuple[torch.Tensor, Overlap]] = []
        for view, view_offsets in targets:
            ov = compute_overlap(
                shard.offsets, shard.sizes, view_offsets, list(view.shape)
            )
            if ov is not None:
                hits.append((view, ov))
        if not hits:
            continue
        byte_range = (
            tuple(shard.tensor.byte_range) if shard.tensor.byte_range else None
        )
        consumer = ShardConsumer(shard_entry=shard.tensor, targets=hits)
        buf_alloc = (
            consumer.alloc_pinned_buffer
            if (
                consumer.all_targets_on_device()
                and shard.tensor.serializer != "torch_save"
            )
            else None
        )
        read_reqs.append(
            ReadReq(
                path=shard.tensor.location,
                consumer=consumer,
                byte_range=byte_range,
                buf_alloc=buf_alloc,
            )
        )
    return read_reqs


# ---------------------------------------------------------------------------
# preparer
# ---------------------------------------------------------------------------


class ShardedTensorIOPreparer:
    @staticmethod
    def prepare_write(
        storage_path: str,
        obj: Any,  # ShardedTensor
        is_async_snapshot: bool = False,
        save_dtype: Optional[torch.dtype] = None,
    ) -> Tuple[ShardedTensorEntry, List[WriteReq]]:
        max_bytes = knobs.get_max_shard_size_bytes()
        shards_meta: List[ShardMeta] = []
        write_reqs: List[WriteReq] = []
        global_shape = list(obj.metadata().size)
        for local_shard in obj.local_shards():
            tensor = local_shard.tensor
            offsets = list(local_shard.metadata.shard_offsets)
            for piece, piece_offsets in subdivide_shard(
                tensor, offsets, max_bytes
            ):
                location = location_for_shard(storage_path, piece_offsets)
                sub_entry, sub_reqs = TensorIOPreparer.prepare_write(
                    storage_path=location,
                    tensor=piece,
                    replicated=False,
                    is_async_snapshot=is_async_snapshot,
                    save_dtype=save_dtype,
                )
                shards_meta.append(
                    ShardMeta(
                        offsets=piece_offsets,
                        sizes=list(piece.shape),
                        tensor=sub_entry,
                    )
                )
                write_reqs.extend(sub_reqs)
        entry = ShardedTensorEntry(
            shards=shards_meta,
            dtype=dtype_to_str(save_dtype or obj.dtype),
            shape=global_shape,
        )
        return entry, write_reqs

    @staticmethod
    def prepare_read(
        entry: ShardedTensorEntry,
        obj_out: Optional[Any] = None,
    ) -> Tuple[List[ReadReq], LoadFuture]:
        try:
            from torch.distributed._shard.sharded_tensor import ShardedTensor
        except ImportError:
            ShardedTensor = ()  # type: ignore[assignment]

        global_shape = entry.shape or _infer_global_shape(entry)

        if isinstance(obj_out, ShardedTensor):
            st_shape = list(obj_out.metadata().size)
            if entry.shape and st_shape != list(entry.shape):
                logger.warning(
                    "global shape mismatch on sharded restore: snapshot %s "
                    "vs target %s; loading the overlap",
                    entry.shape,
                    st_shape,
                )
            targets = [
                (ls.tensor, list(ls.metadata.shard_offsets))
                for ls in obj_out.local_shards()
            ]
            fut = LoadFuture(obj_out)
            return plan_shard_reads(entry.shards, targets), fut

        # load into a plain full tensor (obj_out or a fresh CPU tensor)
        if isinstance(obj_out, torch.Tensor):
            full = obj_out
        else:
            dtype = (
                str_to_dtype(entry.dtype)
                if entry.dtype
                else str_to_dtype(entry.shards[0].tensor.dtype)
            )
            full = torch.empty(global_shape, dtype=dtype)
        targets = [(full, [0] * full.dim())]
        fut = LoadFuture(full)
        return plan_shard_reads(entry.shards, targets), fut


def _infer_global_shape(entry: ShardedTensorEntry) -> List[int]:
    ndim = len(entry.shards[0].offsets)
    shape = [0] * ndim
    for s in entry.shards:
        for d in range(ndim):
            shape[d] = max(shape[d], s.offsets[d] + s.sizes[d])
    return shape
