"""MI355X device staging engine.

Replaces the reference's per-tensor ``tensor.cpu()`` staging
(torchsnapshot/io_preparers/tensor.py:353-355) and its
``GPUBatchedBufferStager`` (torchsnapshot/batcher.py:104-162) with a native
HIP data plane for gfx950:

- a pinned host block pool (D2H lands here; pinned memory is what the SDMA
  engines need to run at full PCIe Gen5 rate, ~55-60 GB/s effective),
- a per-device side HIP stream, so D2H copies and pack-kernel launches
  overlap with whatever the training step has in flight,
- one gather-pack kernel launch per slab: N strided device tensors are
  packed contiguously (256 B aligned each) either into a device slab that
  is then moved by a single SDMA copy, or directly into pinned host memory
  over PCIe (mode knob; both paths are implemented in
  ops/hip/staging.hip).

Failure policy: if a CUDA/HIP tensor must be staged and the compiled
extension is missing, we raise — a silent eager fallback would invalidate
every benchmark above it. Set TSAMD_DISABLE_HIP_STAGING=1 to explicitly opt
into the torch fallback (debug only).
"""

from __future__ import annotations

import contextlib
import math
import threading
from dataclasses import dataclass
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import torch

from .. import knobs

ALIGN = 256  # slab alignment per packed tensor

try:
    from torchsnapshot_amd import _csnap  # compiled HIP extension

    HIP_EXT_AVAILABLE = True
except ImportError:  # CPU-only container, or extension not built yet
    _csnap = None
    HIP_EXT_AVAILABLE = False


def _require_ext() -> None:
    if not HIP_EXT_AVAILABLE:
        raise RuntimeError(
            "torchsnapshot_amd's HIP staging extension (_csnap) is not built "
            "but a device tensor needs staging. Build it with "
            "`python -m torchsnapshot_amd.ops.build` (gfx950), or set "
            "TSAMD_DISABLE_HIP_STAGING=1 to explicitly use the slow torch "
            "fallback."
        )


# ---------------------------------------------------------------------------
# tensor layout descriptors
# ---------------------------------------------------------------------------


def collapse_layout(t: torch.Tensor) -> Tuple[List[int], List[int]]:
    """Collapse a tensor's (sizes, strides) by merging ADJACENT LOGICAL dims
    that are jointly contiguous, dropping size-1 dims. Serialization follows
    the logical (row-major over t.shape) element order — the same bytes
    ``t.contiguous()`` would produce — so dims must NOT be reordered by
    stride. Returns element-unit (sizes, strides), innermost last; a fully
    contiguous tensor collapses to ([numel], [1])."""
    sizes = [s for s, st in zip(t.shape, t.stride()) if s != 1]
    strides = [st for s, st in zip(t.shape, t.stride()) if s != 1]
    if not sizes:
        # scalar or all-size-1 tensor: one element
        return [1], [1]
    merged_sizes: List[int] = [sizes[0]]
    merged_strides: List[int] = [strides[0]]
    for s, st in zip(sizes[1:], strides[1:]):
        # logical-adjacent dims merge iff outer stride == inner stride * size
        if merged_strides[-1] == st * s:
            merged_sizes[-1] *= s
            merged_strides[-1] = st
        else:
            merged_sizes.append(s)
            merged_strides.append(st)
    return merged_sizes, merged_strides


def outer_dim_count(t: torch.Tensor) -> int:
    """Strided dims left for the kernels to decompose after collapsing: all
    collapsed dims but an innermost contiguous row."""
    sizes, strides = collapse_layout(t)
    return len(sizes) - 1 if strides[-1] == 1 else len(sizes)


MAX_OUTER_DIMS = 6  # kMaxDims in ops/hip/desc_check.h


def resolve_lazy(t: torch.Tensor) -> torch.Tensor:
    """``t`` with a lazy conjugate or negative bit applied to its bytes.

    ``x.conj()`` and ``torch._neg_view(x)`` share ``x``'s memory, sizes and
    strides and differ from it only in a flag, so anything that describes
    raw memory has to resolve them first or it saves ``x``. ``detach()``
    and ``contiguous()`` keep the bits. Resolving changes neither numel
    nor dtype, and a tensor without the bits is returned as it is."""
    if t.is_conj():
        t = t.resolve_conj()
    if t.is_neg():
        t = t.resolve_neg()
    return t


@dataclass
class PackItem:
    """One tensor's gather descriptor inside a slab."""

    src_ptr: int          # device base address of element [0,...,0]
    flat_offset: int      # byte offset within the slab
    nbytes: int           # logical payload bytes
    row_bytes: int        # innermost contiguous run in bytes
    outer_sizes: List[int]    # sizes of non-contiguous dims (row-major)
    outer_strides: List[int]  # byte strides of those dims
    vec: int              # safe vector width (16/8/4/2/1)
    # narrowing cast fused into the gather (CAST_* below). With a cast,
    # nbytes/row_bytes/flat_offset/vec are in STORED (destination) bytes;
    # src_ptr and outer_strides stay in source bytes, and a lane reads
    # 2*vec source bytes per vec stored bytes.
    cast: int = 0


CAST_NONE = 0
CAST_F32_TO_BF16 = 1
CAST_F32_TO_F16 = 2

_CAST_CODES = {
    (torch.float32, torch.bfloat16): CAST_F32_TO_BF16,
    (torch.float32, torch.float16): CAST_F32_TO_F16,
}


def cast_code(src: torch.dtype, dst: Optional[torch.dtype]) -> int:
    """Descriptor cast code for storing a ``src``-typed tensor as ``dst``.
    An unsupported pair raises: a tensor is never silently left uncast."""
    if dst is None or dst == src:
        return CAST_NONE
    code = _CAST_CODES.get((src, dst))
    if code is None:
        raise ValueError(
            f"the gather kernel cannot cast {src} to {dst}; supported: "
            "float32 -> bfloat16, float32 -> float16"
        )
    return code


# widening on restore (scatter only): the descriptor convention is the cast
# one, flat side in stored 2-byte units and tensor side in float32 bytes
CAST_BF16_TO_F32 = 3
CAST_F16_TO_F32 = 4

_WIDEN_CODES = {
    (torch.bfloat16, torch.float32): CAST_BF16_TO_F32,
    (torch.float16, torch.float32): CAST_F16_TO_F32,
}


def widen_code(stored: torch.dtype, target: torch.dtype) -> int:
    """Descriptor cast code for restoring ``stored``-typed bytes into a
    ``target``-typed tensor. An unsupported pair raises."""
    if stored == target:
        return CAST_NONE
    code = _WIDEN_CODES.get((stored, target))
    if code is None:
        raise ValueError(
            f"the scatter kernel cannot restore {stored} into {target}; "
            "supported: equal dtypes, bfloat16 -> float32, float16 -> float32"
        )
    return code


def _layout_rows(
    sizes: List[int],
    strides: List[int],
    src_esz: int,
    flat_esz: int,
    data_ptr: int,
) -> Tuple[int, List[int], List[int], int]:
    """Rows of a collapsed element-unit layout, as every descriptor states
    them: ``(row_bytes, outer_sizes, outer_strides_b, src_align)``.

    ``row_bytes`` is the innermost contiguous run in flat-side bytes
    (``flat_esz`` per element; it differs from ``src_esz`` only under a
    cast), the outer strides are tensor-side bytes, and ``src_align`` is the
    largest power of two up to 16 that divides the base address and every
    outer stride (a stride of 0 divides by anything). Each builder derives
    its own vec from these and keeps its own refusals."""
    src_align = math.gcd(16, data_ptr)
    if len(sizes) == 1 and strides[0] == 1:
        return sizes[0] * flat_esz, [], [], src_align  # contiguous: one row
    if strides[-1] == 1:
        row_elems, n_outer = sizes[-1], len(sizes) - 1
    else:
        # innermost dim itself strided: rows of one element
        row_elems, n_outer = 1, len(sizes)
    outer_strides_b = [st * src_esz for st in strides[:n_outer]]
    for st in outer_strides_b:
        src_align = math.gcd(src_align, st if st else 16)
    return row_elems * flat_esz, sizes[:n_outer], outer_strides_b, src_align


def build_pack_items(
    tensors: Sequence[torch.Tensor],
    out_dtypes: Optional[Sequence[Optional[torch.dtype]]] = None,
) -> Tuple[List[PackItem], List[int], int]:
    """Compute slab layout for a batch: per-tensor descriptors, per-tensor
    slab offsets, and total slab bytes (each tensor 256B-aligned).
    ``out_dtypes`` optionally names a stored dtype per tensor; the layout
    (offsets, sizes, total) is then in stored bytes."""
    if out_dtypes is None:
        out_dtypes = [None] * len(tensors)
    if len(out_dtypes) != len(tensors):
        raise ValueError("out_dtypes must have one entry per tensor")
    items: List[PackItem] = []
    offsets: List[int] = []
    off = 0
    for t, out_dtype in zip(tensors, out_dtypes):
        cast = cast_code(t.dtype, out_dtype)
        if cast != CAST_NONE:
            item = _build_cast_item(t, out_dtype, cast, off)
            items.append(item)
            offsets.append(off)
            off += (item.nbytes + ALIGN - 1) // ALIGN * ALIGN
            continue
        nbytes = t.numel() * t.element_size()
        sizes, strides = collapse_layout(t)
        esz = t.element_size()
        if t.numel() == 0:
            items.append(PackItem(t.data_ptr(), off, 0, 0, [], [], 1))
            offsets.append(off)
            continue
        row_bytes, outer_sizes, outer_strides_b, src_align = _layout_rows(
            sizes, strides, esz, esz, t.data_ptr()
        )
        vec = math.gcd(row_bytes, src_align)
        items.append(
            PackItem(
                src_ptr=t.data_ptr(),
                flat_offset=off,
                nbytes=nbytes,
                row_bytes=row_bytes,
                outer_sizes=outer_sizes,
                outer_strides=outer_strides_b,
                vec=vec,
            )
        )
        offsets.append(off)
        off += (nbytes + ALIGN - 1) // ALIGN * ALIGN
    return items, offsets, off


def _build_cast_item(
    t: torch.Tensor, out_dtype: torch.dtype, cast: int, off: int
) -> PackItem:
    """Descriptor of a tensor stored as ``out_dtype``. The flat side is in
    stored bytes; vec is the widest store (16/8/4/2 B) such that the
    matching 2*vec-byte source read splits into naturally aligned loads
    (two 16 B loads at vec 16, else one load of 2*vec)."""
    if t.numel() == 0:
        return PackItem(t.data_ptr(), off, 0, 0, [], [], 1, CAST_NONE)
    src_esz = t.element_size()
    dst_esz = out_dtype.itemsize
    sizes, strides = collapse_layout(t)
    row_bytes, outer_sizes, outer_strides_b, src_align = _layout_rows(
        sizes, strides, src_esz, dst_esz, t.data_ptr()
    )
    if src_align < src_esz:
        raise ValueError(
            f"cannot cast-stage a {t.dtype} tensor whose address or strides "
            f"are not {src_esz}-byte aligned"
        )
    vec = min(math.gcd(16, row_bytes), 16 if src_align == 16 else src_align // 2)
    return PackItem(
        src_ptr=t.data_ptr(),
        flat_offset=off,
        nbytes=t.numel() * dst_esz,
        row_bytes=row_bytes,
        outer_sizes=outer_sizes,
        outer_strides=outer_strides_b,
        vec=vec,
        cast=cast,
    )


def build_scatter_items(
    targets: Sequence[torch.Tensor],
    stored_dtypes: Sequence[torch.dtype],
    flat_offsets: Sequence[int],
    flat_base: int = 0,
) -> List[PackItem]:
    """Descriptors for scattering payload bytes into ``targets`` (restore).

    Unlike a gather, the flat side is not laid out here: member ``i`` sits
    at ``flat_offsets[i]`` (its byte_range within the read), and the flat
    buffer starts at address ``flat_base``. ``vec`` therefore has to divide
    the flat address as well as everything build_pack_items makes it
    divide. A bf16/f16 payload for a float32 target becomes a widen item."""
    items: List[PackItem] = []
    for t, stored, off in zip(targets, stored_dtypes, flat_offsets):
        code = widen_code(stored, t.dtype)
        if code != CAST_NONE:
            it = _build_cast_item(t, stored, code, off)
        else:
            it = build_pack_items([t])[0][0]
            it.flat_offset = off
        if it.nbytes:
            it.vec = math.gcd(it.vec, flat_base + off)
            if it.cast != CAST_NONE and it.vec < 2:
                raise ValueError(
                    f"cannot widen from a payload at odd address "
                    f"{flat_base + off:#x}"
                )
        items.append(it)
    return items


# The extension's cap on one descriptor's flat-side bytes (gather, scatter
# and scan alike; kMaxDescBytes in ops/hip/desc_check.h): u32 indices inside
# the kernels step up to 4 KiB past a tensor's size, so anything closer to
# 4 GiB than one 64 KiB work unit is refused on the host.
_KERNEL_MAX_BYTES = 2**32 - 2**16


def scatter_plan(
    target: torch.Tensor, stored_dtype: torch.dtype
) -> Optional[int]:
    """The descriptor cast code with which the scatter kernel can restore a
    ``stored_dtype`` payload into ``target``, or None when it must not be
    used and the caller keeps the torch path."""
    if target.device.type != "cuda":
        return None
    return _scatter_layout_plan(target, stored_dtype)


def _scatter_layout_plan(
    target: torch.Tensor, stored_dtype: torch.dtype
) -> Optional[int]:
    """scatter_plan() past the device check."""
    if (
        target.layout != torch.strided
        or target.is_quantized
        or target.is_conj()
        or target.is_neg()
    ):
        return None
    if stored_dtype != target.dtype and (
        (stored_dtype, target.dtype) not in _WIDEN_CODES
    ):
        return None
    # overlapping elements: the kernel writes them in no defined order
    if any(st == 0 and sz > 1 for sz, st in zip(target.shape, target.stride())):
        return None
    if torch._debug_has_internal_overlap(target) != 0:
        return None
    if outer_dim_count(target) > MAX_OUTER_DIMS:
        return None
    if target.numel() * stored_dtype.itemsize >= _KERNEL_MAX_BYTES:
        return None
    # torch strides are whole elements, so the base address decides whether
    # every element is aligned
    if target.data_ptr() % target.element_size():
        return None
    return widen_code(stored_dtype, target.dtype)


def scatter_member(
    target: torch.Tensor, stored_dtype: torch.dtype, flat_offset: int
) -> Optional[Tuple[torch.Tensor, torch.dtype, int]]:
    """One StagingEngine.scatter member, or None when this restore has to
    stay on the torch path: TSAMD_RESTORE_MODE=torch, no extension, an
    ineligible target, or a payload offset that splits an element."""
    if (
        knobs.get_restore_mode() == "torch"
        or not HIP_EXT_AVAILABLE
        or knobs.is_hip_staging_disabled()
        or flat_offset % stored_dtype.itemsize
        or scatter_plan(target, stored_dtype) is None
    ):
        return None
    return (target, stored_dtype, flat_offset)


# ---------------------------------------------------------------------------
# non-finite scan descriptors
# ---------------------------------------------------------------------------

# element classes of the scan kernel (kScan* in ops/hip/staging.hip). The
# last two count what a save_dtype narrowing of a float32 tensor will write.
SCAN_F64 = 0
SCAN_F32 = 1
SCAN_F16 = 2
SCAN_BF16 = 3
SCAN_E5M2 = 4
SCAN_E4M3FN = 5
SCAN_FNUZ = 6
SCAN_F32_AS_F16 = 7
SCAN_F32_AS_BF16 = 8

_SCAN_CLASSES: Dict[torch.dtype, int] = {
    torch.float64: SCAN_F64,
    torch.float32: SCAN_F32,
    torch.float16: SCAN_F16,
    torch.bfloat16: SCAN_BF16,
}
for _name, _cls in (
    ("float8_e5m2", SCAN_E5M2),
    ("float8_e4m3fn", SCAN_E4M3FN),
    ("float8_e4m3fnuz", SCAN_FNUZ),
    ("float8_e5m2fnuz", SCAN_FNUZ),
):
    if hasattr(torch, _name):
        _SCAN_CLASSES[getattr(torch, _name)] = _cls

_SCAN_STORED_CLASSES = {
    CAST_F32_TO_F16: SCAN_F32_AS_F16,
    CAST_F32_TO_BF16: SCAN_F32_AS_BF16,
}


def collapse_layout_by_stride(t: torch.Tensor) -> Tuple[List[int], List[int]]:
    """collapse_layout() for consumers that do not care about element order
    (a count): dims are sorted by stride before jointly contiguous
    neighbours merge, so a dense transposed or permuted tensor collapses to
    one run. Stride-0 (expanded) dims are kept, outermost, so every logical
    element is still visited once. Returns element-unit (sizes, strides),
    innermost last; the multiset of addresses they enumerate is the
    tensor's own."""
    dims = [(st, s) for s, st in zip(t.shape, t.stride()) if s != 1]
    if not dims:
        return [1], [1]
    expanded = [d for d in dims if d[0] == 0]
    dense = sorted((d for d in dims if d[0] != 0), reverse=True)
    merged_sizes: List[int] = []
    merged_strides: List[int] = []
    for st, s in expanded + dense:
        if merged_sizes and merged_strides[-1] == st * s:
            merged_sizes[-1] *= s
            merged_strides[-1] = st
        else:
            merged_sizes.append(s)
            merged_strides.append(st)
    return merged_sizes, merged_strides


def scan_class(
    dtype: torch.dtype, stored_dtype: Optional[torch.dtype] = None
) -> Optional[int]:
    """Scan-kernel element class of a real ``dtype`` tensor that will be
    stored as ``stored_dtype`` (None = as is), or None for a dtype that has
    no non-finite values to count."""
    code = cast_code(dtype, stored_dtype) if stored_dtype is not None else CAST_NONE
    if code != CAST_NONE:
        return _SCAN_STORED_CLASSES[code]
    return _SCAN_CLASSES.get(dtype)


def _scan_view(t: torch.Tensor) -> Optional[torch.Tensor]:
    """The real strided view whose elements a scan counts, or None when the
    tensor is not scanned (non-float dtype, quantized, sparse)."""
    if t.is_quantized or t.layout != torch.strided:
        return None
    if t.dtype.is_complex:
        if t.is_conj():
            t = t.conj()  # flips the lazy-conjugate bit: same memory
        t = torch.view_as_real(t)
    return t if t.dtype in _SCAN_CLASSES else None


def _build_scan_item(t: torch.Tensor) -> Optional[PackItem]:
    """Descriptor of one real float view of at most _KERNEL_MAX_BYTES, or
    None when the kernel cannot take it."""
    esz = t.element_size()
    if t.is_neg():
        return None
    sizes, strides = collapse_layout_by_stride(t)
    row_bytes, outer_sizes, outer_strides_b, src_align = _layout_rows(
        sizes, strides, esz, esz, t.data_ptr()
    )
    if len(outer_sizes) > 6:
        return None
    vec = math.gcd(row_bytes, src_align)
    if vec < esz:
        return None  # storage offset splits an element
    return PackItem(
        src_ptr=t.data_ptr(),
        flat_offset=0,
        nbytes=t.numel() * esz,
        row_bytes=row_bytes,
        outer_sizes=outer_sizes,
        outer_strides=outer_strides_b,
        vec=vec,
    )


def build_scan_items(
    tensors: Sequence[torch.Tensor],
    stored_dtypes: Optional[Sequence[Optional[torch.dtype]]] = None,
) -> Tuple[List[Optional[List[PackItem]]], List[Optional[int]]]:
    """Scan-kernel descriptors for a batch, one entry per tensor.

    ``classes[i]`` is the tensor's element class, or None when it is not
    scanned at all (non-float dtype, quantized, sparse). ``items[i]`` is the
    list of descriptors whose counts sum to the tensor's: empty without
    elements, several when the tensor is over the kernel's size cap and was
    split along dim 0. It is None when the builder declines the tensor and
    the caller has to count with torch instead: more than 6 outer dims
    after collapsing, a storage offset that splits an element, or a tensor
    that splitting cannot bring under the cap. A complex tensor is
    described through ``torch.view_as_real``: its counts are of components.
    """
    if stored_dtypes is None:
        stored_dtypes = [None] * len(tensors)
    if len(stored_dtypes) != len(tensors):
        raise ValueError("stored_dtypes must have one entry per tensor")
    items: List[Optional[List[PackItem]]] = []
    classes: List[Optional[int]] = []
    for t, stored in zip(tensors, stored_dtypes):
        view = _scan_view(t)
        cls = None if view is None else scan_class(view.dtype, stored)
        classes.append(cls)
        if cls is None:
            items.append(None)
            continue
        pieces = _split_for_scan(view)
        built = None if pieces is None else [_build_scan_item(p) for p in pieces]
        if built is None or any(it is None for it in built):
            items.append(None)
        else:
            items.append(built)
    return items, classes


def _split_for_scan(t: torch.Tensor) -> Optional[List[torch.Tensor]]:
    """``t`` as views of at most the scan cap each: itself, or dim-0 slices
    of at most the chunk size as the chunker cuts them. None when one dim-0
    row alone is over the cap."""
    if t.numel() == 0:
        return []
    nbytes = t.numel() * t.element_size()
    if nbytes <= _KERNEL_MAX_BYTES:
        return [t]
    if t.dim() == 0:
        return None
    row_bytes = nbytes // t.shape[0]
    max_bytes = min(knobs.get_max_chunk_size_bytes(), _KERNEL_MAX_BYTES)
    if row_bytes > max_bytes:
        return None
    rows = max_bytes // row_bytes
    return [
        t.narrow(0, off, min(rows, t.shape[0] - off))
        for off in range(0, t.shape[0], rows)
    ]


def torch_count_nonfinite(
    t: torch.Tensor, stored_dtype: Optional[torch.dtype] = None
) -> Tuple[int, int]:
    """(NaN, Inf) element counts by the torch expression, on the tensor's
    own device: what the scan kernel must agree with, and the path for
    anything it declines. (0, 0) for tensors that are not scanned."""
    view = _scan_view(t)
    if view is None or view.numel() == 0:
        return (0, 0)
    if scan_class(view.dtype, stored_dtype) in _SCAN_STORED_CLASSES.values():
        view = view.to(stored_dtype)
    elif view.element_size() == 1:
        view = view.to(torch.float32)  # fp8: isnan/isinf want a wider type
    return int(torch.isnan(view).sum()), int(torch.isinf(view).sum())


def _items_to_flat(items: List[PackItem]) -> List[int]:
    """Serialize descriptors for the extension: fixed-width int rows."""
    MAXD = 6
    flat: List[int] = []
    for it in items:
        if len(it.outer_sizes) > MAXD:
            raise ValueError(
                f"tensor layout too complex to pack ({len(it.outer_sizes)} "
                "outer dims after collapsing; max 6)"
            )
        row = [
            it.src_ptr,
            it.flat_offset,
            it.nbytes,
            it.row_bytes,
            it.vec,
            len(it.outer_sizes),
        ]
        sizes = list(it.outer_sizes) + [1] * (MAXD - len(it.outer_sizes))
        strides = list(it.outer_strides) + [0] * (MAXD - len(it.outer_strides))
        row += sizes + strides
        row.append(it.cast)
        flat += row
    return flat


# ---------------------------------------------------------------------------
# pinned host pool
# ---------------------------------------------------------------------------


class PinnedBlock:
    def __init__(self, tensor: torch.Tensor, pooled: bool) -> None:
        self.tensor = tensor  # 1-D uint8, pin_memory=True
        self.pooled = pooled

    @property
    def nbytes(self) -> int:
        return self.tensor.numel()


class PinnedPool:
    """Fixed pool of pinned host blocks; oversized requests get a one-off
    pinned allocation. acquire() blocks until a block frees up, which
    naturally backpressures staging against storage-write drain."""

    def __init__(
        self, block_size: Optional[int] = None, block_count: Optional[int] = None
    ) -> None:
        self.block_size = block_size or knobs.get_pinned_block_size_bytes()
        self.max_blocks = block_count or knobs.get_pinned_block_count()
        self._free: List[torch.Tensor] = []
        self._allocated = 0
        self._cond = threading.Condition()

    def _alloc(self, nbytes: int) -> torch.Tensor:
        """Every block's memory comes from here."""
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)

    def acquire(self, nbytes: int) -> PinnedBlock:
        if nbytes > self.block_size:
            return PinnedBlock(self._alloc(nbytes), pooled=False)
        with self._cond:
            while True:
                if self._free:
                    return PinnedBlock(self._free.pop(), pooled=True)
                if self._allocated < self.max_blocks:
                    self._allocated += 1
                    break
                self._cond.wait()
        return PinnedBlock(self._alloc(self.block_size), pooled=True)

    def release(self, block: PinnedBlock) -> None:
        if not block.pooled:
            return  # one-off allocation; freed by GC
        with self._cond:
            self._free.append(block.tensor)
            self._cond.notify()

    def prealloc_one(self) -> bool:
        """Allocate one new block straight into the free list (never takes
        from it), so warming can proceed concurrently with real staging
        without hoarding blocks."""
        with self._cond:
            if self._allocated >= self.max_blocks:
                return False
            self._allocated += 1
        tensor = self._alloc(self.block_size)
        with self._cond:
            self._free.append(tensor)
            self._cond.notify()
        return True


_pool_lock = threading.Lock()
_pool: Optional[PinnedPool] = None


def get_pinned_pool() -> PinnedPool:
    global _pool
    with _pool_lock:
        if _pool is None:
            _pool = PinnedPool()
        return _pool


_warm_stop = threading.Event()
_warm_thread: Optional[threading.Thread] = None
# [pool, bytes] the warming thread still has to pin (pool_warming_paused)
_warm_left: list = [None, 0]


def _join_warm_thread() -> None:
    # a pinned allocation in flight during interpreter teardown aborts the
    # process (HIP resources die under the daemon thread); stop between
    # blocks and join before exit
    _warm_stop.set()
    t = _warm_thread
    if t is not None and t.is_alive():
        t.join(timeout=30)


def warm_pinned_pool(nbytes: Optional[int] = None, background: bool = True) -> None:
    """Pre-allocate (and so pre-register) pinned blocks. Pinning is a
    one-time ~GB/s kernel-side cost; warming it off the critical path
    keeps the FIRST checkpoint as fast as the rest (measured 14.4 s ->
    0.35 s first-async-take stall for an 8 GB model). Called automatically
    (in the background) when a StagingEngine is first created."""
    _start_warming(get_pinned_pool(), nbytes, background)


@contextlib.contextmanager
def pool_warming_paused() -> Iterator[None]:
    """Hold background pool warming for the duration: the warming thread
    stops after the block it is pinning, and what it had left to warm is
    warmed in the background again afterwards. Pinned allocations take a
    runtime-wide lock; this is for code that must not share it (a latency
    measurement, a test of one)."""
    t = _warm_thread
    paused = t is not None and t.is_alive()
    if paused:
        _warm_stop.set()
        t.join()
        _warm_stop.clear()
    try:
        yield
    finally:
        if paused and _warm_left[1] > 0:
            _start_warming(_warm_left[0], _warm_left[1], background=True)


def _start_warming(
    pool: PinnedPool, nbytes: Optional[int], background: bool
) -> None:
    global _warm_thread

    def work() -> None:
        import os

        if nbytes is not None:
            target = nbytes
        else:
            # default: don't pin the whole pool for workloads that may
            # never need it — 8 GB covers most first checkpoints
            target = min(
                pool.block_size * pool.max_blocks,
                int(float(os.environ.get("TSAMD_POOL_WARM_BYTES", 8 * 1024**3))),
            )
        allocated = 0
        _warm_left[:] = [pool, target]
        while (
            not _warm_stop.is_set()
            and allocated < target
            and pool.prealloc_one()
        ):
            allocated += pool.block_size
            _warm_left[1] = target - allocated
        if not _warm_stop.is_set():
            _warm_left[1] = 0  # done, or the pool is full

    if background:
        import atexit

        with _pool_lock:
            if _warm_thread is not None and _warm_thread.is_alive():
                return
            _warm_thread = threading.Thread(
                target=work, name="tsamd-pool-warm", daemon=True
            )
            atexit.register(_join_warm_thread)
            _warm_thread.start()
    else:
        work()


# ---------------------------------------------------------------------------
# staging engine
# ---------------------------------------------------------------------------


@dataclass
class StagedBatch:
    """Handle for one in-flight D2H staging operation."""

    pinned: PinnedBlock
    offsets: List[int]
    nbytes_list: List[int]
    total_bytes: int
    _handle: Optional[int] = None          # _csnap op handle
    _device_slab: Optional[torch.Tensor] = None  # keep alive until done
    # per-tensor psum64 values (device-computed), populated at wait() when
    # checksumming was requested
    checksums: Optional[List[int]] = None
    _hash_tensor: Optional[torch.Tensor] = None
    # source tensors referenced until the async gather/copy completes, so
    # callers may drop theirs right after stage()
    _sources: Optional[Sequence[torch.Tensor]] = None
    _done: bool = False

    def wait(self) -> None:
        """Block until the D2H copy has landed in pinned memory."""
        if self._done:
            return
        if self._handle is not None:
            _csnap.wait(self._handle)
            self._handle = None
        if self._hash_tensor is not None:
            self.checksums = [int(v) for v in self._hash_tensor.cpu().tolist()]
            self._hash_tensor = None
        self._device_slab = None
        self._sources = None
        self._done = True

    def memoryview_of(self, index: int) -> memoryview:
        assert self._done, "wait() before reading staged buffers"
        off = self.offsets[index]
        n = self.nbytes_list[index]
        if n == 0:
            return memoryview(b"")
        return memoryview(self.pinned.tensor.numpy())[off : off + n]

    def slab_memoryview(self) -> memoryview:
        assert self._done
        return memoryview(self.pinned.tensor.numpy())[: self.total_bytes]

    def release(self) -> None:
        get_pinned_pool().release(self.pinned)


class StagingEngine:
    """Per-device staging front end. Thread-safe; all GPU work goes to the
    extension's side stream for the device."""

    def __init__(self, device: torch.device) -> None:
        self.device = device
        self._use_ext = HIP_EXT_AVAILABLE and not knobs.is_hip_staging_disabled()
        if not self._use_ext and not knobs.is_hip_staging_disabled():
            _require_ext()
        # hide the one-time pinned-registration cost behind whatever runs
        # before the first checkpoint
        warm_pinned_pool()

    def stage(
        self,
        tensors: Sequence[torch.Tensor],
        compute_checksums: bool = False,
        out_dtypes: Optional[Sequence[Optional[torch.dtype]]] = None,
    ) -> StagedBatch:
        """Start async D2H staging of device tensors into one pinned slab.

        ``out_dtypes`` optionally gives a stored dtype per tensor (None =
        as is). A float32 tensor with a bfloat16/float16 target is narrowed
        inside the gather kernel: offsets, sizes and checksums of the batch
        are then those of the stored bytes. Other pairs raise ValueError.

        With ``compute_checksums``, the gather kernel also accumulates a
        psum64 checksum per tensor at no measurable cost (the kernel is
        PCIe-bound); padding gaps are zeroed so the sum of the per-tensor
        values is the checksum of the whole written file.

        The caller must ensure the tensors' producing stream is
        torch.cuda.current_stream() of this thread (true for checkpointing:
        tensors are live parameters/opt states, already materialized)."""
        # descriptors state raw memory: a lazily conjugated or negated
        # tensor is saved by value. The pack kernel indexes within-tensor
        # bytes as u32 and decomposes at most 6 outer dims: materialize
        # non-contiguous tensors over 2 GiB or beyond 6 dims first
        # (chunking splits along dim 0 upstream, and such layouts are
        # rare). The stride>=0 check is defensive only — torch itself
        # forbids negative strides.
        tensors = [resolve_lazy(t) for t in tensors]
        tensors = [
            t
            if (
                t.is_contiguous()
                or (
                    t.numel() * t.element_size() < 2**31
                    and all(s >= 0 for s in t.stride())
                    and outer_dim_count(t) <= MAX_OUTER_DIMS
                )
            )
            else t.contiguous()
            for t in tensors
        ]
        items, offsets, total = build_pack_items(tensors, out_dtypes)
        nbytes_list = [it.nbytes for it in items]
        pinned = get_pinned_pool().acquire(max(total, 1))
        batch = StagedBatch(
            pinned=pinned,
            offsets=offsets,
            nbytes_list=nbytes_list,
            total_bytes=total,
        )
        if total == 0:
            batch._done = True
            return batch
        batch._sources = tensors
        try:
            if self._use_ext:
                self._stage_ext(
                    tensors, items, batch, total,
                    compute_checksums=compute_checksums,
                )
            else:
                self._stage_torch_fallback(tensors, items, batch, out_dtypes)
        except BaseException:
            # don't leak the pool slot on launch failure
            get_pinned_pool().release(pinned)
            raise
        return batch

    # -- native path --------------------------------------------------------

    def _stage_ext(
        self,
        tensors: Sequence[torch.Tensor],
        items: List[PackItem],
        batch: StagedBatch,
        total: int,
        compute_checksums: bool = False,
    ) -> None:
        dev_index = self.device.index or 0
        with torch.cuda.device(dev_index):
            cur_stream = torch.cuda.current_stream().cuda_stream
            single_contig = (
                len(items) == 1
                and not items[0].outer_sizes
                and items[0].cast == CAST_NONE
                and not compute_checksums
            )
            if single_contig:
                # one SDMA copy, no kernel
                handle = _csnap.d2h_copy(
                    items[0].src_ptr,
                    batch.pinned.tensor.data_ptr(),
                    items[0].nbytes,
                    cur_stream,
                    dev_index,
                )
            else:
                mode = _pack_mode()
                slab = None
                slab_ptr = 0
                hash_ptr = 0
                if compute_checksums:
                    # padding must read as zeros so per-tensor checksums
                    # sum to the file checksum
                    batch._hash_tensor = torch.zeros(
                        len(items), dtype=torch.uint64, device=self.device
                    )
                    hash_ptr = batch._hash_tensor.data_ptr()
                if mode == "slab":
                    slab = (
                        torch.zeros(total, dtype=torch.uint8, device=self.device)
                        if compute_checksums
                        else torch.empty(
                            total, dtype=torch.uint8, device=self.device
                        )
                    )
                    slab_ptr = slab.data_ptr()
                elif compute_checksums:
                    # direct mode: kernel writes only payload bytes; zero
                    # the pinned gap regions host-side (tiny)
                    pin_np = batch.pinned.tensor.numpy()
                    prev_end = 0
                    for it in items:
                        if it.flat_offset > prev_end:
                            pin_np[prev_end : it.flat_offset] = 0
                        prev_end = it.flat_offset + it.nbytes
                    if total > prev_end:
                        pin_np[prev_end:total] = 0
                handle = _csnap.pack_d2h(
                    _items_to_flat(items),
                    len(items),
                    slab_ptr,
                    batch.pinned.tensor.data_ptr(),
                    total,
                    cur_stream,
                    dev_index,
                    hash_ptr,
                )
                batch._device_slab = slab
            batch._handle = handle

    # -- restore ------------------------------------------------------------

    def scatter(
        self,
        pinned_block: PinnedBlock,
        nbytes: int,
        members: Sequence[Tuple[torch.Tensor, torch.dtype, int]],
        expected_psum: Optional[Tuple[int, int]] = None,
        what: str = "payload",
    ) -> None:
        """Restore the first ``nbytes`` of ``pinned_block`` into device
        tensors with ONE scatter-kernel launch. ``members`` holds
        ``(target, stored_dtype, flat_offset)`` triples, each eligible per
        scatter_plan(); bf16/f16 payloads widen into float32 targets inside
        the kernel. Returns once the targets hold the bytes, so the caller
        may release the block.

        ``expected_psum=(value, word_base)``: the kernel also accumulates
        the psum64 of every member's payload bytes, at file offset
        ``word_base * 8`` for the block's first byte, and their sum is
        checked against ``value``. The targets have already been written
        when the mismatch is raised."""
        if not self._use_ext:
            _require_ext()
            raise RuntimeError("scatter() needs the HIP staging extension")
        members = [m for m in members if m[0].numel() > 0]
        if not members:
            if expected_psum is not None and expected_psum[0] != 0:
                _raise_psum_mismatch(what, expected_psum[0], 0)
            return
        dev_index = self.device.index or 0
        base = pinned_block.tensor.data_ptr()
        items = build_scatter_items(
            [m[0] for m in members],
            [m[1] for m in members],
            [m[2] for m in members],
            flat_base=base,
        )
        with torch.cuda.device(dev_index):
            cur_stream = torch.cuda.current_stream().cuda_stream
            slab = None
            if knobs.get_restore_mode() == "slab":
                slab = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            hash_t = None
            if expected_psum is not None:
                hash_t = torch.zeros(
                    len(items), dtype=torch.uint64, device=self.device
                )
            handle = _csnap.unpack_h2d(
                _items_to_flat(items),
                len(items),
                slab.data_ptr() if slab is not None else 0,
                base,
                nbytes,
                cur_stream,
                dev_index,
                hash_t.data_ptr() if hash_t is not None else 0,
                expected_psum[1] * 8 if expected_psum is not None else 0,
            )
            _csnap.wait(handle)
            if hash_t is not None:
                got = sum(int(v) for v in hash_t.cpu().tolist()) % (1 << 64)
                if got != expected_psum[0]:
                    _raise_psum_mismatch(what, expected_psum[0], got)

    # -- non-finite scan ----------------------------------------------------

    def scan_nonfinite(
        self,
        tensors: Sequence[torch.Tensor],
        stored_dtypes: Optional[Sequence[Optional[torch.dtype]]] = None,
    ) -> List[Tuple[int, int]]:
        """(NaN, Inf) element counts of each of this device's ``tensors``,
        from ONE read-only scan-kernel launch over all of them. Blocking.

        Counts are of logical elements: they equal ``torch.isnan(t).sum()``
        and ``torch.isinf(t).sum()`` for any layout (an expanded dim counts
        as often as torch counts it), of components for complex tensors.
        With ``stored_dtypes[i]`` bfloat16/float16 for a float32 tensor they
        are the counts of ``t.to(stored)``: what a save_dtype snapshot will
        hold. Non-float, quantized and sparse tensors report (0, 0).

        Tensors build_scan_items() declines are counted with the torch
        expression instead; so is everything when the extension is disabled
        by TSAMD_DISABLE_HIP_STAGING=1."""
        if stored_dtypes is None:
            stored_dtypes = [None] * len(tensors)
        if not self._use_ext:
            return [
                torch_count_nonfinite(t, st)
                for t, st in zip(tensors, stored_dtypes)
            ]
        per_tensor, classes = build_scan_items(tensors, stored_dtypes)
        flat_items: List[PackItem] = []
        flat_classes: List[int] = []
        owners: List[int] = []
        for i, (its, cls) in enumerate(zip(per_tensor, classes)):
            for it in its or ():
                flat_items.append(it)
                flat_classes.append(cls)
                owners.append(i)
        out = [[0, 0] for _ in tensors]
        if flat_items:
            dev_index = self.device.index or 0
            with torch.cuda.device(dev_index):
                counts = _csnap.scan_nonfinite(
                    _items_to_flat(flat_items),
                    flat_classes,
                    len(flat_items),
                    torch.cuda.current_stream().cuda_stream,
                    dev_index,
                )
            for k, i in enumerate(owners):
                out[i][0] += int(counts[2 * k])
                out[i][1] += int(counts[2 * k + 1])
        for i, (its, cls) in enumerate(zip(per_tensor, classes)):
            if cls is not None and its is None:
                out[i] = list(
                    torch_count_nonfinite(tensors[i], stored_dtypes[i])
                )
        return [(a, b) for a, b in out]

    # -- debug fallback -----------------------------------------------------

    def _stage_torch_fallback(
        self,
        tensors: Sequence[torch.Tensor],
        items: List[PackItem],
        batch: StagedBatch,
        out_dtypes: Optional[Sequence[Optional[torch.dtype]]] = None,
    ) -> None:
        if out_dtypes is None:
            out_dtypes = [None] * len(items)
        for t, it, out_dtype in zip(tensors, items, out_dtypes):
            if it.nbytes == 0:
                continue
            if it.cast != CAST_NONE:
                t = t.to(out_dtype)
            flat = t.contiguous().reshape(-1).view(torch.uint8)
            dst = batch.pinned.tensor[it.flat_offset : it.flat_offset + it.nbytes]
            dst.copy_(flat, non_blocking=True)
        torch.cuda.synchronize(self.device)
        batch._done = True


def _pack_mode() -> str:
    # "direct": the gather kernel writes straight into pinned host memory
    # over PCIe (measured ~50 GB/s on MI355X, and +20% on the full
    # checkpoint bench vs the device-slab + SDMA hop, which also costs a
    # transient slab allocation per batch). "slab" keeps CU time minimal
    # (kernel runs at HBM speed, SDMA does the PCIe leg) for overlap with
    # heavy training compute.
    import os

    mode = os.environ.get("TSAMD_STAGE_MODE", "direct")
    if mode not in ("slab", "direct"):
        raise ValueError(f"TSAMD_STAGE_MODE must be slab|direct, got {mode}")
    return mode


def device_psum64(dev_u8: torch.Tensor, file_byte_off: int = 0) -> int:
    """psum64 of a contiguous uint8 device tensor, computed on-device at
    HBM speed (restore-verification path; ~free vs the H2D copy that
    produced the bytes). ``file_byte_off`` is the byte offset of the
    buffer's first byte within its payload file (8-aligned)."""
    _require_ext()
    assert dev_u8.dtype == torch.uint8 and dev_u8.is_contiguous()
    assert dev_u8.device.type == "cuda"
    if dev_u8.numel() == 0:
        return 0
    return int(
        _csnap.psum64_dev(
            dev_u8.data_ptr(),
            dev_u8.numel(),
            file_byte_off,
            torch.cuda.current_stream(dev_u8.device).cuda_stream,
            dev_u8.device.index,
        )
    )


def verify_device_psum(
    dev_u8: torch.Tensor, expected: "tuple[int, int]", what: str
) -> None:
    """Check a device buffer against (expected_psum_value, word_base);
    raises like the CPU verifier on mismatch."""
    value, word_base = expected
    got = device_psum64(dev_u8, word_base * 8)
    if got != value:
        _raise_psum_mismatch(what, value, got)


def _raise_psum_mismatch(what: str, value: int, got: int) -> None:
    raise RuntimeError(
        f"checksum mismatch for '{what}': snapshot recorded "
        f"psum64:{value:016x}, device read back psum64:{got:016x} — "
        "the file is corrupted or was modified after the snapshot "
        "was committed"
    )


_engines: Dict[int, StagingEngine] = {}
_engines_lock = threading.Lock()


def get_staging_engine(device: torch.device) -> StagingEngine:
    idx = device.index if device.index is not None else torch.cuda.current_device()
    with _engines_lock:
        if idx not in _engines:
            _engines[idx] = StagingEngine(torch.device("cuda", idx))
        return _engines[idx]
