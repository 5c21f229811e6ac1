"""Tensor I/O preparer: the core of the data path.

Write: a device tensor is staged through the HIP engine (gather-pack kernel
+ SDMA D2H into pinned memory, ops/staging.py); a CPU tensor is exposed
zero-copy (cloned only when required for safety). Read: buffer bytes are
wrapped zero-copy and scattered into the destination tensor in-place,
with optional tiled reads that bound peak host memory for huge tensors.

Parity with reference torchsnapshot/io_preparers/tensor.py (staging rules
:240-307, tiled reads :128-181, quantized-aware copy :385-409) with an
MI355X-native staging mechanism.
"""

from __future__ import annotations

import asyncio
from typing import Any, List, Optional, Tuple

import torch

from ..io_types import (
    BufferStager,
    BufferType,
    ReadReq,
    StageContext,
    WriteReq,
)
from .. import integrity
from ..manifest import TensorEntry
from ..ops.staging import (
    HIP_EXT_AVAILABLE,
    get_staging_engine,
    resolve_lazy,
    scatter_member,
)
from ..serialization import (
    SERIALIZER_BUFFER,
    SERIALIZER_QTENSOR,
    SERIALIZER_TORCH_SAVE,
    dtype_to_str,
    pick_serializer,
    qtensor_as_bytes,
    qtensor_from_bytes,
    str_to_dtype,
    tensor_as_memoryview,
    tensor_from_memoryview,
    torch_load_from_bytes,
    torch_save_as_bytes,
)
from .pinned_read import PinnedReadConsumer, payload_to_device, view_payload


class LoadFuture:
    """Resolved once the read pipeline completes; .obj is the loaded value."""

    __slots__ = ["obj"]

    def __init__(self, obj: Any = None) -> None:
        self.obj = obj


def tensor_copy(dst: torch.Tensor, src: torch.Tensor) -> None:
    """Copy src into dst in-place, handling dtype/device casts and
    quantization-scheme mismatches."""
    dst = dst.detach()
    if src.is_quantized and not dst.is_quantized:
        src = src.dequantize()
    if dst.is_quantized and not src.is_quantized:
        raise ValueError(
            "cannot load a non-quantized payload into a quantized tensor "
            f"(dst dtype {dst.dtype})"
        )
    if (
        dst.is_quantized
        and src.is_quantized
        and dst.qscheme() != src.qscheme()
    ):
        raise ValueError(
            f"quantization scheme mismatch: dst {dst.qscheme()} vs src "
            f"{src.qscheme()}"
        )
    dst.copy_(src)


class TensorIOPreparer:
    @staticmethod
    def prepare_write(
        storage_path: str,
        tensor: torch.Tensor,
        replicated: bool = False,
        is_async_snapshot: bool = False,
        save_dtype: Optional[torch.dtype] = None,
    ) -> Tuple[TensorEntry, List[WriteReq]]:
        """``save_dtype`` stores the tensor narrowed to that dtype (the
        entry records the STORED dtype); it requires the plain buffer
        serializer."""
        serializer = pick_serializer(tensor)
        if save_dtype == tensor.dtype:
            save_dtype = None
        if save_dtype is not None and serializer != SERIALIZER_BUFFER:
            raise ValueError(
                f"save_dtype={save_dtype} needs a buffer-serialized tensor, "
                f"got serializer '{serializer}' for dtype {tensor.dtype}"
            )
        entry = TensorEntry(
            location=storage_path,
            serializer=serializer,
            dtype=dtype_to_str(save_dtype or tensor.dtype),
            shape=list(tensor.shape),
            replicated=replicated,
        )
        stager = TensorBufferStager(
            tensor=tensor,
            serializer=serializer,
            is_async_snapshot=is_async_snapshot,
            save_dtype=save_dtype,
        )
        return entry, [
            WriteReq(path=storage_path, stager=stager, tensor_entry=entry)
        ]

    @staticmethod
    def prepare_read(
        entry: TensorEntry,
        tensor_out: Optional[torch.Tensor] = None,
        buffer_size_limit_bytes: Optional[int] = None,
    ) -> Tuple[List[ReadReq], LoadFuture]:
        nbytes = entry.nbytes_estimate()
        if (
            buffer_size_limit_bytes is not None
            and entry.serializer == SERIALIZER_BUFFER
            and entry.byte_range is None
            and nbytes > buffer_size_limit_bytes
        ):
            return TensorIOPreparer._prepare_read_tiled(
                entry, tensor_out, buffer_size_limit_bytes
            )
        fut = LoadFuture(tensor_out)
        consumer = TensorBufferConsumer(entry=entry, tensor_out=tensor_out, fut=fut)
        byte_range = tuple(entry.byte_range) if entry.byte_range else None
        # device targets read straight into pinned memory (if the request
        # ends up merged into a batched span, the span read ignores this
        # and the consumer falls back to the bounce path)
        buf_alloc = (
            consumer.alloc_pinned_buffer
            if (
                tensor_out is not None
                and tensor_out.device.type == "cuda"
                and entry.serializer == SERIALIZER_BUFFER
            )
            else None
        )
        return [
            ReadReq(
                path=entry.location,
                consumer=consumer,
                byte_range=byte_range,
                buf_alloc=buf_alloc,
            )
        ], fut

    @staticmethod
    def _prepare_read_tiled(
        entry: TensorEntry,
        tensor_out: Optional[torch.Tensor],
        limit: int,
    ) -> Tuple[List[ReadReq], LoadFuture]:
        """Split one big buffer-serialized tensor into byte-ranged reads so
        peak host memory stays under ``limit`` (random-access API)."""
        dtype = str_to_dtype(entry.dtype)
        nbytes = entry.nbytes_estimate()
        elem = max(dtype.itemsize, 1)
        # tiles write straight into the output when it is contiguous with a
        # matching dtype — on ANY device (CUDA tiles go pinned -> SDMA H2D,
        # so peak host memory stays at the budget, never the tensor size)
        direct = (
            tensor_out is not None
            and tensor_out.is_contiguous()
            and tensor_out.dtype == dtype
        )
        staging = (
            tensor_out
            if direct
            else torch.empty(entry.shape, dtype=dtype)
        )
        fut = LoadFuture(tensor_out if tensor_out is not None else staging)
        flat_u8 = staging.reshape(-1).view(torch.uint8) if nbytes else None
        tile = max(limit - limit % elem, elem)
        reqs: List[ReadReq] = []
        state = _TiledReadState(
            remaining=(nbytes + tile - 1) // tile if nbytes else 0,
            staging=staging,
            tensor_out=None if direct else tensor_out,
        )
        for start in range(0, nbytes, tile):
            end = min(start + tile, nbytes)
            consumer = _TensorTileConsumer(
                dst_flat_u8=flat_u8, start=start, end=end, state=state
            )
            reqs.append(
                ReadReq(
                    path=entry.location,
                    byte_range=(start, end),
                    consumer=consumer,
                    buf_alloc=(
                        consumer.alloc_pinned_buffer
                        if staging.device.type == "cuda"
                        else None
                    ),
                )
            )
        if not reqs:  # empty tensor
            if tensor_out is not None and not direct:
                tensor_copy(tensor_out, staging)
        return reqs, fut


class _TiledReadState:
    def __init__(
        self,
        remaining: int,
        staging: torch.Tensor,
        tensor_out: Optional[torch.Tensor],
    ) -> None:
        self.remaining = remaining
        self.staging = staging
        self.tensor_out = tensor_out
        self.lock = __import__("threading").Lock()


class _TensorTileConsumer(PinnedReadConsumer):
    def __init__(
        self,
        dst_flat_u8: torch.Tensor,
        start: int,
        end: int,
        state: _TiledReadState,
    ) -> None:
        self.dst_flat_u8 = dst_flat_u8
        self.start = start
        self.end = end
        self.state = state

    def get_consuming_cost_bytes(self) -> int:
        return self.end - self.start

    async def consume_buffer(self, ctx: StageContext, buf: BufferType) -> None:
        def work() -> None:
            n = self.end - self.start
            if self._pinned_block is not None:
                src = self._pinned_block.tensor[:n]  # pinned: async-capable
            else:
                src = torch.frombuffer(buf, dtype=torch.uint8)
            self.dst_flat_u8[self.start : self.end].copy_(src)
            with self.state.lock:
                self.state.remaining -= 1
                last = self.state.remaining == 0
            if last and self.state.tensor_out is not None:
                tensor_copy(self.state.tensor_out, self.state.staging)

        await asyncio.get_running_loop().run_in_executor(ctx.executor, work)


class TensorBufferStager(BufferStager):
    def __init__(
        self,
        tensor: torch.Tensor,
        serializer: str,
        is_async_snapshot: bool = False,
        save_dtype: Optional[torch.dtype] = None,
    ) -> None:
        self.tensor = tensor
        self.serializer = serializer
        self.is_async_snapshot = is_async_snapshot
        # stored dtype when it differs from the tensor's (narrowing save):
        # device tensors are cast inside the gather kernel, host tensors
        # with torch in _stage_cpu
        self.save_dtype = save_dtype
        self._staged_batch = None  # StagedBatch for device tensors

    def stored_nbytes(self) -> int:
        """Payload bytes as written (after the save_dtype cast, if any)."""
        esz = (
            self.save_dtype.itemsize
            if self.save_dtype is not None
            else self.tensor.element_size()
        )
        return self.tensor.numel() * esz

    def get_staging_cost_bytes(self) -> int:
        nbytes = self.stored_nbytes()
        if self.serializer in (SERIALIZER_TORCH_SAVE, SERIALIZER_QTENSOR):
            # these serializers materialize a second copy while packing
            return 2 * nbytes
        return nbytes

    async def stage_buffer(self, ctx: StageContext) -> BufferType:
        loop = asyncio.get_running_loop()
        if self.tensor.device.type == "cuda":
            return await loop.run_in_executor(ctx.executor, self._stage_device)
        return await loop.run_in_executor(ctx.executor, self._stage_cpu, ctx)

    def _stage_device(self) -> BufferType:
        from ..uvm_tensor import is_uvm_tensor, uvm_to_cpu

        # a lazy conj/neg view is saved by value, on every branch below
        t = resolve_lazy(self.tensor.detach())
        if t.is_quantized or self.serializer != SERIALIZER_BUFFER:
            # rare path: bring to host with torch, then pack
            cpu = t.cpu()
            if self.serializer == SERIALIZER_QTENSOR:
                return qtensor_as_bytes(cpu)
            return torch_save_as_bytes(cpu)
        if is_uvm_tensor(t):
            # managed memory is CPU-addressable: serialize zero-copy, no
            # D2H needed (clone when async: training may mutate the pages)
            cpu = uvm_to_cpu(t)
            if self.save_dtype is not None:
                # the cast result is already a private copy
                return tensor_as_memoryview(
                    cpu.to(self.save_dtype).contiguous()
                )
            if self.is_async_snapshot:
                cpu = cpu.clone()
            return tensor_as_memoryview(cpu.contiguous())
        engine = get_staging_engine(t.device)
        ck = integrity.checksumming_enabled()
        batch = engine.stage(
            [t],
            compute_checksums=ck,
            out_dtypes=None if self.save_dtype is None else [self.save_dtype],
        )
        batch.wait()  # blocks in executor thread; GIL released inside HIP
        if ck and batch.checksums is not None:
            self.precomputed_checksum = integrity.format_psum64(batch.checksums[0])
        self._staged_batch = batch
        return batch.memoryview_of(0)

    def _stage_cpu(self, ctx: StageContext) -> BufferType:
        # resolved first: tensor_as_memoryview cannot view a lazy conj/neg
        # tensor's bytes, and they would be the unresolved ones
        src = self.tensor.detach()
        t = resolve_lazy(src)
        if self.serializer == SERIALIZER_QTENSOR:
            return qtensor_as_bytes(t)
        if self.serializer == SERIALIZER_TORCH_SAVE:
            return torch_save_as_bytes(t)
        if self.save_dtype is not None:
            # runs on the executor thread; the cast result is a private
            # copy, so async snapshots need no extra clone
            return tensor_as_memoryview(t.to(self.save_dtype).contiguous())
        # a resolved lazy view is a private copy already
        if t is src and self._should_copy_cpu_tensor(t, ctx):
            t = t.contiguous().clone() if not t.is_contiguous() else t.clone()
        elif not t.is_contiguous():
            t = t.contiguous()
        return tensor_as_memoryview(t)

    def _should_copy_cpu_tensor(self, t: torch.Tensor, ctx: StageContext) -> bool:
        # Async snapshots: training resumes (and may mutate the tensor) as
        # soon as staging completes, so the bytes handed to storage must be
        # a private copy.
        if self.is_async_snapshot:
            return True
        # A view over a larger storage: serializing zero-copy would leak
        # unrelated bytes lifetimes; cheaper to copy the logical content.
        if t.numel() * t.element_size() != t.untyped_storage().nbytes():
            return True
        return False

    def release_buffer(self) -> None:
        if self._staged_batch is not None:
            self._staged_batch.release()
            self._staged_batch = None
        # drop the source reference: for shadow-cloned async saves this
        # frees the device clone as soon as its write completes (any
        # zero-copy host buffer stays alive through the memoryview)
        self.tensor = None  # type: ignore[assignment]


class TensorBufferConsumer(PinnedReadConsumer):
    def __init__(
        self,
        entry: TensorEntry,
        tensor_out: Optional[torch.Tensor],
        fut: LoadFuture,
    ) -> None:
        self.entry = entry
        self.tensor_out = tensor_out
        self.fut = fut

    def get_consuming_cost_bytes(self) -> int:
        nbytes = self.entry.nbytes_estimate()
        if self.entry.serializer == SERIALIZER_TORCH_SAVE:
            return 2 * nbytes
        return nbytes

    def device_span_target(self):
        if (
            self.tensor_out is not None
            and self.tensor_out.device.type == "cuda"
            and self.entry.serializer == SERIALIZER_BUFFER
        ):
            return self.tensor_out.device
        return None

    def will_verify_on_device(self) -> bool:
        # only the pinned -> device path checksums on the GPU
        return (
            HIP_EXT_AVAILABLE
            and self._pinned_block is not None
            and self.device_span_target() is not None
        )

    def scatter_members(self, base_offset: int, verified: bool = False):
        """The one member covers the payload exactly once, which is what a
        ``verified`` scatter asks for."""
        out = self.tensor_out
        if (
            out is None
            or self.entry.serializer != SERIALIZER_BUFFER
            # copy_ would broadcast a differently shaped payload
            or list(out.shape) != list(self.entry.shape)
        ):
            return None
        member = scatter_member(
            out.detach(), str_to_dtype(self.entry.dtype), base_offset
        )
        return None if member is None else [member]

    def consume_from_device_u8(self, dev_u8: torch.Tensor) -> None:
        loaded = view_payload(
            dev_u8, str_to_dtype(self.entry.dtype), self.entry.shape
        )
        tensor_copy(self.tensor_out, loaded)
        self.fut.obj = self.tensor_out

    async def consume_buffer(self, ctx: StageContext, buf: BufferType) -> None:
        def work() -> None:
            out = self.tensor_out
            if self.entry.serializer == SERIALIZER_QTENSOR:
                loaded = qtensor_from_bytes(buf)
            elif self.entry.serializer == SERIALIZER_TORCH_SAVE:
                loaded = torch_load_from_bytes(bytes(buf))
            elif out is not None and out.device.type == "cuda":
                dev_u8 = payload_to_device(
                    self,
                    buf,
                    out.device,
                    self.scatter_members(0)
                    if self._pinned_block is not None
                    else None,
                    self.expected_psum,
                    self.entry.location,
                )
                if dev_u8 is None:  # the scatter kernel wrote the target
                    self.fut.obj = out
                    return
                return self.consume_from_device_u8(dev_u8)
            else:
                loaded = tensor_from_memoryview(
                    memoryview(buf),
                    dtype=str_to_dtype(self.entry.dtype),
                    shape=tuple(self.entry.shape),
                )
            if out is not None:
                tensor_copy(out, loaded)
                self.fut.obj = out
            else:
                self.fut.obj = loaded

        await asyncio.get_running_loop().run_in_executor(ctx.executor, work)
