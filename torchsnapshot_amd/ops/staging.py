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
import struct
import threading
from dataclasses import dataclass
from typing import Any, Callable, Dict, Iterator, List, Optional, Sequence, Tuple

import torch

from .. import knobs
from ..serialization import MXFP4_E2M1, MXFP8_E4M3, is_mx, mx_nbytes

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

    @property
    def stored_bytes(self) -> int:
        """Payload bytes in the slab: ``nbytes``, and for a block-scaled
        item the scale bytes that follow the codes region."""
        if self.cast >= CAST_F32_TO_MX4:
            return self.nbytes + self.nbytes // (MX_BLOCK // 2)
        if self.cast >= CAST_F32_TO_MX:
            return self.nbytes + self.nbytes // MX_BLOCK
        return self.nbytes


CAST_NONE = 0
CAST_F32_TO_BF16 = 1
CAST_F32_TO_F16 = 2

# Block-scaled fp8 and fp4 (docs/format.md). They are no torch dtypes:
# wherever a stored dtype is named, their strings stand for them
# (serialization.is_mx).
MX_BLOCK = 32
CAST_F32_TO_MX = 16
CAST_BF16_TO_MX = 17
CAST_F32_TO_MX4 = 20
CAST_BF16_TO_MX4 = 21

StoredDtype = Any  # a torch.dtype, MXFP8_E4M3 or MXFP4_E2M1

_CAST_CODES = {
    (torch.float32, torch.bfloat16): CAST_F32_TO_BF16,
    (torch.float32, torch.float16): CAST_F32_TO_F16,
    (torch.float32, MXFP8_E4M3): CAST_F32_TO_MX,
    (torch.bfloat16, MXFP8_E4M3): CAST_BF16_TO_MX,
    (torch.float32, MXFP4_E2M1): CAST_F32_TO_MX4,
    (torch.bfloat16, MXFP4_E2M1): CAST_BF16_TO_MX4,
}


def stored_nbytes(numel: int, dtype: StoredDtype) -> int:
    """Payload bytes of ``numel`` elements stored as ``dtype``: per block of
    32, 33 bytes for block-scaled fp8 and 17 for fp4."""
    if is_mx(dtype):
        return mx_nbytes(numel, dtype)
    return numel * dtype.itemsize


def cast_code(src: torch.dtype, dst: Optional[StoredDtype]) -> int:
    """Descriptor cast code for storing a ``src``-typed tensor as ``dst``.
    An unsupported pair raises: a tensor is never silently left uncast."""
    if dst is None or dst == src:
        return CAST_NONE
    code = _CAST_CODES.get((src, dst))
    if code is None:
        raise ValueError(
            f"the gather kernel cannot cast {src} to {dst}; supported: "
            "float32 -> bfloat16, float32 -> float16, float32 or bfloat16 "
            f"-> {MXFP8_E4M3!r} or {MXFP4_E2M1!r}"
        )
    return code


def _pow2(k: torch.Tensor) -> torch.Tensor:
    """2^k in float64 for an int64 tensor with |k| < 1023, built from the
    bit pattern: exact on every device."""
    return ((k + 1023) << 52).view(torch.float64)


def _mx_blocks(t: torch.Tensor) -> torch.Tensor:
    """``t``'s row-major elements in float64 as (blocks, 32), the last block
    padded with zeros."""
    x = resolve_lazy(t.detach()).reshape(-1).to(torch.float64)
    nb = (x.numel() + MX_BLOCK - 1) // MX_BLOCK
    if x.numel() != nb * MX_BLOCK:
        x = torch.cat([x, x.new_zeros(nb * MX_BLOCK - x.numel())])
    return x.reshape(nb, MX_BLOCK)


def mx_encode(t: torch.Tensor) -> torch.Tensor:
    """The mxfp8_e4m3 payload of ``t`` (float32 or bfloat16, any layout) as
    a uint8 tensor on ``t``'s device: 32 code bytes per block of its
    row-major elements, then one scale byte per block (docs/format.md). The
    torch expression of what the gather kernel stores, byte for byte."""
    x = _mx_blocks(t)
    finite = torch.isfinite(x)
    amax = torch.where(finite, x.abs(), 0.0).amax(dim=1)
    # amax = m * 2^e with m in [0.5, 1): floor(log2 amax) is e - 1
    exp = torch.frexp(amax).exponent.to(torch.int64) - 9
    exp = exp + (amax * _pow2(-exp) > 448.0).to(torch.int64)
    exp = torch.where(amax == 0, -127, exp).clamp_(min=-127)
    y = (torch.where(finite, x, 0.0) * _pow2(-exp)[:, None]).clamp_(-448.0, 448.0)
    codes = y.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)
    nan_code = torch.signbit(x).to(torch.uint8) * 0x80 + 0x7F
    codes = torch.where(finite, codes, nan_code)
    return torch.cat([codes.reshape(-1), (exp + 127).to(torch.uint8)])


def mx_decode(payload: torch.Tensor, n: int, dtype: torch.dtype) -> torch.Tensor:
    """The ``n`` elements of an mxfp8_e4m3 ``payload`` (uint8, 33 bytes per
    block) as a 1-D ``dtype`` tensor on its device: code times 2^(X - 127),
    exact in float32, then rounded to ``dtype``; a scale byte of 0xFF gives
    NaN. The torch expression of what the scatter kernel restores."""
    nb = (n + MX_BLOCK - 1) // MX_BLOCK
    if payload.numel() != 33 * nb:
        raise ValueError(
            f"mxfp8_e4m3 payload of {n} elements must be {33 * nb} bytes, "
            f"got {payload.numel()}"
        )
    codes = payload[: MX_BLOCK * nb].view(torch.float8_e4m3fn).to(torch.float32)
    scale = payload[MX_BLOCK * nb :].to(torch.int64) - 127
    x = codes.to(torch.float64).reshape(nb, MX_BLOCK) * _pow2(scale)[:, None]
    # the MX rule: a scale byte of 0xFF makes the whole block NaN
    x = torch.where((scale == 128)[:, None], float("nan"), x)
    return x.reshape(-1)[:n].to(torch.float32).to(dtype)


def mx4_encode(t: torch.Tensor) -> torch.Tensor:
    """The mxfp4_e2m1 payload of ``t`` (float32 or bfloat16, any layout) as
    a uint8 tensor on ``t``'s device: 16 code bytes per block of its
    row-major elements, the even element in the low nibble, then one scale
    byte per block (docs/format.md). The torch expression of what the gather
    kernel stores, byte for byte."""
    x = _mx_blocks(t)
    finite = torch.isfinite(x)
    amax = torch.where(finite, x.abs(), 0.0).amax(dim=1)
    # amax = m * 2^e with m in [0.5, 1): floor(log2 amax) is e - 1
    exp = torch.frexp(amax).exponent.to(torch.int64) - 3
    exp = exp + (amax * _pow2(-exp) > 6.0).to(torch.int64)
    exp = torch.where(amax == 0, -127, exp).clamp_(min=-127)
    y = torch.where(finite, x, 0.0).abs() * _pow2(-exp)[:, None]
    # the code is the number of grid midpoints at or below y; a midpoint
    # itself goes to the even code, so every other comparison is strict
    mag = sum(
        (y >= mid) if k % 2 else (y > mid)
        for k, mid in enumerate((0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0))
    )
    mag = torch.where(finite, mag, 7).to(torch.uint8)
    codes = mag + torch.signbit(x).to(torch.uint8) * 8
    packed = codes[:, 0::2] | (codes[:, 1::2] << 4)
    scales = torch.where(finite.all(dim=1), exp + 127, 255).to(torch.uint8)
    return torch.cat([packed.reshape(-1), scales])


_E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mx4_decode(payload: torch.Tensor, n: int, dtype: torch.dtype) -> torch.Tensor:
    """The ``n`` elements of an mxfp4_e2m1 ``payload`` (uint8, 17 bytes per
    block) as a 1-D ``dtype`` tensor on its device: grid value times
    2^(X - 127), exact in float32 and in bfloat16; a scale byte of 0xFF gives
    NaN. The torch expression of what the scatter kernel restores."""
    nb = (n + MX_BLOCK - 1) // MX_BLOCK
    if payload.numel() != 17 * nb:
        raise ValueError(
            f"mxfp4_e2m1 payload of {n} elements must be {17 * nb} bytes, "
            f"got {payload.numel()}"
        )
    packed = payload[: 16 * nb]
    codes = torch.stack([packed & 0xF, packed >> 4], dim=1).reshape(nb, MX_BLOCK)
    grid = torch.tensor(_E2M1_GRID, dtype=torch.float64, device=payload.device)
    values = grid[(codes & 7).long()] * (1.0 - 2.0 * (codes >> 3).double())
    scale = payload[16 * nb :].to(torch.int64) - 127
    x = values * _pow2(scale)[:, None]
    x = torch.where((scale == 128)[:, None], float("nan"), x)
    return x.reshape(-1)[:n].to(torch.float32).to(dtype)


def mx_encode_as(t: torch.Tensor, stored: str) -> torch.Tensor:
    """``t``'s payload in the block-scaled format ``stored``."""
    return mx4_encode(t) if stored == MXFP4_E2M1 else mx_encode(t)


def mx_decode_as(
    payload: torch.Tensor, stored: str, n: int, dtype: torch.dtype
) -> torch.Tensor:
    """The ``n`` elements of a ``payload`` in the block-scaled format
    ``stored`` as a 1-D ``dtype`` tensor."""
    decode = mx4_decode if stored == MXFP4_E2M1 else mx_decode
    return decode(payload, n, dtype)


# widening on restore (scatter only): the descriptor convention is the cast
# one, flat side in stored 2-byte units and tensor side in float32 bytes
CAST_BF16_TO_F32 = 3
CAST_F16_TO_F32 = 4
# decoding block-scaled fp8: flat side in code bytes, tensor side in target
# bytes
CAST_MX_TO_F32 = 18
CAST_MX_TO_BF16 = 19
CAST_MX4_TO_F32 = 22
CAST_MX4_TO_BF16 = 23

_WIDEN_CODES = {
    (torch.bfloat16, torch.float32): CAST_BF16_TO_F32,
    (torch.float16, torch.float32): CAST_F16_TO_F32,
    (MXFP8_E4M3, torch.float32): CAST_MX_TO_F32,
    (MXFP8_E4M3, torch.bfloat16): CAST_MX_TO_BF16,
    (MXFP4_E2M1, torch.float32): CAST_MX4_TO_F32,
    (MXFP4_E2M1, torch.bfloat16): CAST_MX4_TO_BF16,
}


def widen_code(stored: StoredDtype, target: torch.dtype) -> int:
    """Descriptor cast code for restoring ``stored``-typed bytes into a
    ``target``-typed tensor. An unsupported pair raises."""
    if stored == target:
        return CAST_NONE
    code = _WIDEN_CODES.get((stored, target))
    if code is None:
        raise ValueError(
            f"the scatter kernel cannot restore {stored} into {target}; "
            "supported: equal dtypes, bfloat16 -> float32, float16 -> float32, "
            f"{MXFP8_E4M3!r} or {MXFP4_E2M1!r} -> float32 or bfloat16"
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


def _per_tensor_dtypes(
    dtypes: Optional[Sequence[Optional[torch.dtype]]], n: int, name: str
) -> Sequence[Optional[torch.dtype]]:
    """An optional per-tensor stored-dtype argument as one entry per tensor
    (None = stored as it is)."""
    if dtypes is None:
        return [None] * n
    if len(dtypes) != n:
        raise ValueError(f"{name} must have one entry per tensor")
    return dtypes


def _split_dim0(
    t: torch.Tensor, nbytes: int, piece_bytes: int
) -> Optional[List[torch.Tensor]]:
    """``t``, of ``nbytes`` > 0 stored bytes, as dim-0 slices of at most
    ``piece_bytes`` stored bytes each: the pieces of a tensor that is too
    large for one descriptor of a read-only kernel. None when dim 0 cannot
    cut it that small: a 0-dim tensor, or one row alone over
    ``piece_bytes``."""
    if t.dim() == 0 or nbytes // t.shape[0] > piece_bytes:
        return None
    rows = piece_bytes // (nbytes // t.shape[0])
    return [
        t.narrow(0, off, min(rows, t.shape[0] - off))
        for off in range(0, t.shape[0], rows)
    ]


def build_pack_items(
    tensors: Sequence[torch.Tensor],
    out_dtypes: Optional[Sequence[Optional[torch.dtype]]] = None,
) -> Tuple[List[PackItem], List[int], int]:
    """Compute slab layout for a batch: per-tensor descriptors, per-tensor
    slab offsets, and total slab bytes (each tensor 256B-aligned).
    ``out_dtypes`` optionally names a stored dtype per tensor; the layout
    (offsets, sizes, total) is then in stored bytes."""
    out_dtypes = _per_tensor_dtypes(out_dtypes, len(tensors), "out_dtypes")
    items: List[PackItem] = []
    offsets: List[int] = []
    off = 0
    for t, out_dtype in zip(tensors, out_dtypes):
        cast = cast_code(t.dtype, out_dtype)
        if cast != CAST_NONE:
            item = _build_cast_item(t, out_dtype, cast, off)
            items.append(item)
            offsets.append(off)
            off += (item.stored_bytes + ALIGN - 1) // ALIGN * ALIGN
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
    if is_mx(out_dtype):
        return _build_mx_item(t, out_dtype, cast, off)
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


def _build_mx_item(t: torch.Tensor, stored: str, cast: int, off: int) -> PackItem:
    """Descriptor of a tensor stored as, or restored from, the block-scaled
    format ``stored``. ``nbytes`` is the codes region, 32 bytes per block for
    fp8 (one code byte per element) and 16 for fp4 (two elements per byte),
    and ``row_bytes`` the innermost run in elements. ``vec`` names the kernel
    class: 8, four lanes per block with 16-byte tensor-side accesses, for a
    contiguous tensor or rows of 32k elements whose base and strides are
    16-byte aligned; 1, one lane per block, for every other layout."""
    esz = t.element_size()
    sizes, strides = collapse_layout(t)
    row_elems, outer_sizes, outer_strides_b, src_align = _layout_rows(
        sizes, strides, esz, 1, t.data_ptr()
    )
    if src_align < esz:
        raise ValueError(
            f"cannot stage a {t.dtype} tensor as {stored} whose address or "
            f"strides are not {esz}-byte aligned"
        )
    aligned = src_align == 16 and (not outer_sizes or row_elems % MX_BLOCK == 0)
    blocks = (t.numel() + MX_BLOCK - 1) // MX_BLOCK
    return PackItem(
        src_ptr=t.data_ptr(),
        flat_offset=off,
        nbytes=mx_nbytes(t.numel(), stored) - blocks,  # all but the scales
        row_bytes=row_elems,
        outer_sizes=outer_sizes,
        outer_strides=outer_strides_b,
        vec=8 if aligned else 1,
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
        if it.nbytes and is_mx(stored):
            # codes and scales move as 16-byte pieces; vec names the class
            if (flat_base + off) % 16:
                raise ValueError(
                    f"cannot decode {stored} from a payload at address "
                    f"{flat_base + off:#x}: not 16-byte aligned"
                )
        elif it.nbytes:
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
    # a block-scaled payload's elements are indexed in u32 as well, and fp4
    # has more elements than bytes
    span = target.numel() if is_mx(stored_dtype) else 0
    if max(span, stored_nbytes(target.numel(), stored_dtype)) >= _KERNEL_MAX_BYTES:
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
        or flat_offset % (16 if is_mx(stored_dtype) else stored_dtype.itemsize)
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
    if len(outer_sizes) > MAX_OUTER_DIMS:
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
    stored_dtypes = _per_tensor_dtypes(stored_dtypes, len(tensors), "stored_dtypes")
    items: List[Optional[List[PackItem]]] = []
    classes: List[Optional[int]] = []
    for t, stored in zip(tensors, stored_dtypes):
        view = _scan_view(t)
        cls = None if view is None else scan_class(view.dtype, stored)
        classes.append(cls)
        if cls is None:
            items.append(None)
            continue
        nbytes = view.numel() * view.element_size()
        if nbytes == 0:
            items.append([])
            continue
        pieces: Optional[List[torch.Tensor]] = [view]
        if nbytes > _KERNEL_MAX_BYTES:
            # cut as the chunker would cut it
            pieces = _split_dim0(
                view,
                nbytes,
                min(knobs.get_max_chunk_size_bytes(), _KERNEL_MAX_BYTES),
            )
        built = None if pieces is None else [_build_scan_item(p) for p in pieces]
        if built is None or any(it is None for it in built):
            items.append(None)
        else:
            items.append(built)
    return items, classes


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


# ---------------------------------------------------------------------------
# fingerprint descriptors
# ---------------------------------------------------------------------------


def build_fingerprint_items(
    tensors: Sequence[torch.Tensor],
    stored_dtypes: Optional[Sequence[Optional[torch.dtype]]] = None,
    split_bytes: Optional[int] = None,
) -> List[Optional[List[PackItem]]]:
    """Fingerprint-kernel descriptors for a batch, one entry per tensor.

    They are the gather's descriptors (cast ones for a float32 tensor
    stored as bfloat16/float16) with ``flat_offset`` turned into the byte
    offset at which the piece is hashed: 0 for a whole tensor. A tensor
    whose stored size reaches ``split_bytes`` (default: the kernel's cap)
    is cut along dim 0 into pieces at cumulative stored offsets, with vec
    reduced to divide the offset; psum64 is additive over disjoint byte
    ranges, so the piece sums add up (mod 2^64) to the whole tensor's. An
    entry is ``[]`` for a tensor without elements and None when the builder
    declines and the caller hashes on the host: a quantized or sparse
    tensor, a lazy conjugate or negative view (descriptors state raw memory;
    StagingEngine.fingerprint resolves those first), a stored dtype the
    kernel cannot cast to, elements that are not aligned to their size, more
    than MAX_OUTER_DIMS strided dims, or a tensor at the cap that dim 0
    cannot split."""
    stored_dtypes = _per_tensor_dtypes(stored_dtypes, len(tensors), "stored_dtypes")
    if split_bytes is None:
        split_bytes = _KERNEL_MAX_BYTES
    out: List[Optional[List[PackItem]]] = []
    for t, stored in zip(tensors, stored_dtypes):
        if (
            t.is_quantized
            or t.layout != torch.strided
            or t.is_conj()
            or t.is_neg()
        ):
            out.append(None)
            continue
        t = t.detach()
        if stored == t.dtype:
            stored = None
        if (
            (stored is not None and (t.dtype, stored) not in _CAST_CODES)
            or t.data_ptr() % t.element_size()
        ):
            out.append(None)
            continue
        if t.numel() == 0:
            out.append([])
            continue
        nbytes = t.numel() * (stored or t.dtype).itemsize
        pieces: Optional[List[torch.Tensor]] = [t]
        if nbytes >= split_bytes:
            pieces = _split_dim0(t, nbytes, split_bytes)
        if pieces is None or any(
            outer_dim_count(p) > MAX_OUTER_DIMS for p in pieces
        ):
            out.append(None)
            continue
        items, _, _ = build_pack_items(pieces, [stored] * len(pieces))
        off = 0
        for it in items:
            it.flat_offset = off
            it.vec = math.gcd(it.vec, off) if off else it.vec
            off += it.nbytes
        out.append(items)
    return out


def host_fingerprint(
    t: torch.Tensor, stored_dtype: Optional[torch.dtype] = None
) -> int:
    """psum64 of the bytes ``t`` is stored as, computed on the host: what
    the fingerprint kernel must agree with, and the path for host tensors
    and for anything build_fingerprint_items() declines."""
    from ..integrity import psum64_value

    t = t.detach()
    if t.is_quantized:
        t = t.int_repr()
    if t.layout != torch.strided:
        t = t.to_dense()
    t = resolve_lazy(t)
    if stored_dtype is not None:
        t = t.to(stored_dtype)
    if t.numel() == 0:
        return 0
    flat = t.contiguous().cpu().reshape(-1).view(torch.uint8)
    return psum64_value(flat.numpy())


# ---------------------------------------------------------------------------
# tensor statistics: descriptors, the six words, host fallbacks
# ---------------------------------------------------------------------------

# Six u64 words per tensor, over its finite elements (stats_kernel in
# ops/hip/staging.hip): n_finite, n_zero, minimum and maximum as keys, sum
# and sum of squares as float64 bit patterns. The classes are the first four
# of the scan's: the dtypes that widen to float64 exactly.
_STATS_CLASSES = {
    dt: cls for dt, cls in _SCAN_CLASSES.items() if cls <= SCAN_BF16
}
_M64 = (1 << 64) - 1
# no finite element: the minimum key all ones, the maximum key zero
STATS_EMPTY = (0, 0, _M64, 0, 0, 0)


def stats_key(x: float) -> int:
    """Order-preserving u64 image of a finite float64: keys compare as
    unsigned integers the way the values compare (-0.0 below +0.0)."""
    (b,) = struct.unpack("<Q", struct.pack("<d", x))
    return b ^ (_M64 if b >> 63 else 1 << 63)


def stats_unkey(key: int) -> float:
    b = key ^ (1 << 63 if key >> 63 else _M64)
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def _f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _f64_of(bits: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def merge_stats(a: Sequence[int], b: Sequence[int]) -> List[int]:
    """The six words of two disjoint sets of elements taken together: counts
    add, keys take min / max, the sums add as float64, ``a`` first."""
    return [
        a[0] + b[0],
        a[1] + b[1],
        min(a[2], b[2]),
        max(a[3], b[3]),
        _f64_bits(_f64_of(a[4]) + _f64_of(b[4])),
        _f64_bits(_f64_of(a[5]) + _f64_of(b[5])),
    ]


def decode_stats(words: Sequence[int]) -> Dict[str, Any]:
    """``{n_finite, n_zero, min, max, sum, sumsq}`` of six words; ``min``
    and ``max`` are None when there is no finite element."""
    some = words[0] > 0
    return {
        "n_finite": words[0],
        "n_zero": words[1],
        "min": stats_unkey(words[2]) if some else None,
        "max": stats_unkey(words[3]) if some else None,
        "sum": _f64_of(words[4]),
        "sumsq": _f64_of(words[5]),
    }


def _stats_view(t: torch.Tensor) -> Optional[torch.Tensor]:
    """The tensor whose elements the statistics are of, or None when it
    gets none: fp8, complex, integer, quantized and sparse tensors."""
    if t.is_quantized or t.layout != torch.strided:
        return None
    return t.detach() if t.dtype in _STATS_CLASSES else None


def build_stats_items(
    tensors: Sequence[torch.Tensor],
) -> Tuple[List[Optional[List[PackItem]]], List[Optional[int]]]:
    """Stats-kernel descriptors for a batch, one entry per tensor: the
    scan's descriptors (collapsed in stride order, since no statistic
    depends on element order) under build_scan_items' conventions.
    ``classes[i]`` is None for a tensor that gets no statistics;
    ``items[i]`` is ``[]`` without elements, several descriptors for a
    tensor over the kernel's size cap (their words merge), and None when
    the builder declines and the caller computes with torch: a lazy
    negative view, more than 6 outer dims after collapsing, a storage
    offset that splits an element, or a tensor that dim 0 cannot split."""
    items: List[Optional[List[PackItem]]] = []
    classes: List[Optional[int]] = []
    for t in tensors:
        view = _stats_view(t)
        classes.append(None if view is None else _STATS_CLASSES[view.dtype])
        if view is None:
            items.append(None)
            continue
        nbytes = view.numel() * view.element_size()
        if nbytes == 0:
            items.append([])
            continue
        pieces: Optional[List[torch.Tensor]] = [view]
        if nbytes > _KERNEL_MAX_BYTES:
            pieces = _split_dim0(
                view,
                nbytes,
                min(knobs.get_max_chunk_size_bytes(), _KERNEL_MAX_BYTES),
            )
        built = None if pieces is None else [_build_scan_item(p) for p in pieces]
        if built is None or any(it is None for it in built):
            items.append(None)
        else:
            items.append(built)
    return items, classes


def torch_tensor_stats(
    t: torch.Tensor, stored_dtype: Optional[torch.dtype] = None
) -> List[int]:
    """The six words by torch expressions in float64, on the tensor's own
    device: what the stats kernel must agree with (exactly in the counts,
    minimum and maximum; to rounding in the sums), and the path for
    anything it declines. STATS_EMPTY for a tensor that gets no statistics.
    ``stored_dtype`` is ignored: statistics are of the live values."""
    view = _stats_view(t)
    if view is None:
        return list(STATS_EMPTY)
    x = resolve_lazy(view).to(torch.float64).reshape(-1)
    x = x[torch.isfinite(x)]
    if x.numel() == 0:
        return list(STATS_EMPTY)
    return [
        x.numel(),
        int((x == 0).sum()),
        stats_key(float(x.min())),
        stats_key(float(x.max())),
        _f64_bits(float(x.sum())),
        _f64_bits(float((x * x).sum())),
    ]


def host_tensor_stats(
    t: torch.Tensor, stored_dtype: Optional[torch.dtype] = None
) -> List[int]:
    """torch_tensor_stats() on the host: the path for host tensors."""
    return torch_tensor_stats(t.detach().cpu(), stored_dtype)


# ---------------------------------------------------------------------------
# exponent histograms: the 280 words, host fallbacks
# ---------------------------------------------------------------------------

# HIST_WORDS u64 words per tensor (hist_kernel in ops/hip/staging.hip):
# n_zero (+0 and -0), n_negative (finite, non-zero, sign set), n_nonfinite,
# then for k = 0..276 the finite non-zero elements with
# floor(log2|x|) == k + HIST_MIN_EXP. The bins are float32's binades,
# subnormal ones included; a float64 element outside counts in the end bin.
# words[0] + words[2] + sum(words[3:]) is the element count. Descriptors and
# classes are the statistics' (build_stats_items); all words are counts, so
# the words of disjoint sets of elements add.
HIST_WORDS = 280
HIST_MIN_EXP = -149
HIST_MAX_EXP = 127


def decode_hist(words: Sequence[int]) -> Dict[str, Any]:
    """``{n, n_zero, n_negative, n_nonfinite, bins}`` of the 280 words;
    ``bins`` is ``{floor(log2|x|): count}`` for the non-empty bins."""
    bins = {k + HIST_MIN_EXP: int(c) for k, c in enumerate(words[3:]) if c}
    return {
        "n": int(words[0]) + int(words[2]) + sum(bins.values()),
        "n_zero": int(words[0]),
        "n_negative": int(words[1]),
        "n_nonfinite": int(words[2]),
        "bins": bins,
    }


def torch_tensor_hist(
    t: torch.Tensor, stored_dtype: Optional[torch.dtype] = None
) -> List[int]:
    """The 280 words by torch expressions, on the tensor's own device: what
    the histogram kernel must agree with exactly, and the path for anything
    it declines. The binade comes from ``torch.frexp`` of the values in
    float64, which holds all four dtypes exactly and in which a float32 or
    16-bit subnormal is a normal number. All zeros for a tensor that gets no
    histogram. ``stored_dtype`` is ignored: the values are the live ones."""
    view = _stats_view(t)
    if view is None:
        return [0] * HIST_WORDS
    x = resolve_lazy(view).to(torch.float64).reshape(-1)
    finite = torch.isfinite(x)
    counted = x[finite & (x != 0)]
    # |x| = m * 2^e with m in [0.5, 1): floor(log2|x|) is e - 1
    k = (torch.frexp(counted).exponent.to(torch.int64) - 1 - HIST_MIN_EXP).clamp_(
        0, HIST_MAX_EXP - HIST_MIN_EXP
    )
    bins = torch.bincount(k, minlength=HIST_WORDS - 3)
    return [
        int((x == 0).sum()),
        int((counted < 0).sum()),
        int((~finite).sum()),
        *bins.tolist(),
    ]


def host_tensor_hist(
    t: torch.Tensor, stored_dtype: Optional[torch.dtype] = None
) -> List[int]:
    """torch_tensor_hist() on the host: the path for host tensors."""
    return torch_tensor_hist(t.detach().cpu(), stored_dtype)


# ---------------------------------------------------------------------------
# compare: descriptors, the six fields, the torch expression
# ---------------------------------------------------------------------------

# Six fields per tensor, stored payload s against live tensor v
# (compare_kernel in ops/hip/staging.hip): [n, n_diff, n_nonfinite_diff,
# max_abs, sum_sq, ref_sum_sq]. The last three are floats over the pairs with
# both sides finite, and None for dtypes that are compared bitwise only.
# Element classes (kCmp* in ops/hip/desc_check.h): the stats classes for
# equal float dtypes, raw by element size, and the two widen pairs.
_CMP_RAW_CLASSES = {1: 4, 2: 5, 4: 6, 8: 7, 16: 8}
_CMP_WIDEN_CLASSES = {CAST_BF16_TO_F32: 9, CAST_F16_TO_F32: 10}
_CMP_FIRST_RAW, _CMP_LAST_RAW = 4, 8

Member = Tuple[torch.Tensor, torch.dtype, int]  # live view, stored dtype, flat offset


def compare_class(live: torch.Tensor, stored_dtype: torch.dtype) -> Optional[int]:
    """The compare kernel's element class for a ``stored_dtype`` payload
    against ``live``, or None when the kernel must not be used and the
    caller takes torch_tensor_diff(). It declines what scatter_plan()
    declines, for the same reasons, except internal overlap of the tensor:
    nothing is written, and an element that is visited twice is compared
    twice, as torch does."""
    if (
        live.device.type != "cuda"
        or live.layout != torch.strided
        or live.is_quantized
        or live.is_conj()
        or live.is_neg()
    ):
        return None
    if stored_dtype != live.dtype:
        cls = _CMP_WIDEN_CLASSES.get(_WIDEN_CODES.get((stored_dtype, live.dtype)))
    else:
        cls = _STATS_CLASSES.get(live.dtype, _CMP_RAW_CLASSES.get(live.element_size()))
    if (
        cls is None
        or outer_dim_count(live) > MAX_OUTER_DIMS
        or live.numel() * stored_dtype.itemsize >= _KERNEL_MAX_BYTES
        or live.data_ptr() % live.element_size()
    ):
        return None
    return cls


def build_compare_items(
    members: Sequence[Member], flat_base: int = 0
) -> Tuple[List[Optional[PackItem]], List[Optional[int]]]:
    """Compare-kernel descriptors and classes for the members of one read,
    one entry each: the scatter's descriptors (``vec`` divides the flat
    address ``flat_base + offset`` too). Both entries are None for a member
    the kernel declines: see compare_class(), or a payload address that
    splits a stored element."""
    items: List[Optional[PackItem]] = []
    classes: List[Optional[int]] = []
    for live, stored, off in members:
        cls = compare_class(live, stored)
        item = None
        if cls is not None and (flat_base + off) % stored.itemsize == 0:
            (item,) = build_scatter_items([live], [stored], [off], flat_base)
            if item.nbytes and item.vec < stored.itemsize:
                item = None
        items.append(item)
        classes.append(cls if item is not None else None)
    return items, classes


def decode_diff(words: Sequence[int], cls: int) -> List[Any]:
    """The six fields of the kernel's six words for a descriptor of class
    ``cls``."""
    if _CMP_FIRST_RAW <= cls <= _CMP_LAST_RAW:
        return [words[0], words[1], 0, None, None, None]
    return list(words[:3]) + [_f64_of(w) for w in words[3:6]]


def torch_tensor_diff(stored: torch.Tensor, live: torch.Tensor) -> List[Any]:
    """The six fields by torch expressions in float64, on ``live``'s device:
    what the compare kernel must agree with (exactly but for the two sums,
    which agree to rounding), and the path for host tensors and for
    everything the kernel declines. ``stored`` has ``live``'s shape; it is
    brought to ``live``'s dtype first, and quantized tensors are compared
    dequantized."""
    live = resolve_lazy(live.detach())
    stored = resolve_lazy(stored.detach()).to(live.device)
    if live.layout != torch.strided:
        live = live.to_dense()
    if stored.layout != torch.strided:
        stored = stored.to_dense()
    if live.is_quantized:
        live = live.dequantize()
    if stored.is_quantized:
        stored = stored.dequantize()
    stored = stored.to(live.dtype)
    n = live.numel()
    if n == 0:
        zero = 0.0 if live.dtype in _STATS_CLASSES else None
        return [0, 0, 0, zero, zero, zero]
    esz = live.element_size()
    s_bytes = stored.contiguous().reshape(-1).view(torch.uint8).reshape(n, esz)
    v_bytes = live.contiguous().reshape(-1).view(torch.uint8).reshape(n, esz)
    differ = (s_bytes != v_bytes).any(dim=1)
    n_diff = int(differ.sum())
    if live.dtype not in _STATS_CLASSES:
        return [n, n_diff, 0, None, None, None]
    s = stored.reshape(-1).to(torch.float64)
    v = live.reshape(-1).to(torch.float64)
    both = torch.isfinite(s) & torch.isfinite(v)
    d = (v - s)[both]
    ref = s[both]
    return [
        n,
        n_diff,
        int((differ & ~both).sum()),
        float(d.abs().max()) if d.numel() else 0.0,
        float((d * d).sum()),
        float((ref * ref).sum()),
    ]


def merge_diff(a: Sequence[Any], b: Sequence[Any]) -> List[Any]:
    """The six fields of two disjoint sets of pairs taken together: counters
    add, the maximum is the larger, the sums add as float64, ``a`` first.
    A numeric field is None when it is None on either side."""
    out: List[Any] = [a[0] + b[0], a[1] + b[1], a[2] + b[2]]
    for i, op in ((3, max), (4, float.__add__), (5, float.__add__)):
        out.append(None if a[i] is None or b[i] is None else op(a[i], b[i]))
    return out


def _items_to_flat(items: List[PackItem]) -> List[int]:
    """Serialize descriptors for the extension: fixed-width int rows."""
    flat: List[int] = []
    for it in items:
        if len(it.outer_sizes) > MAX_OUTER_DIMS:
            raise ValueError(
                f"tensor layout too complex to pack ({len(it.outer_sizes)} "
                f"outer dims after collapsing; max {MAX_OUTER_DIMS})"
            )
        row = [
            it.src_ptr,
            it.flat_offset,
            it.nbytes,
            it.row_bytes,
            it.vec,
            len(it.outer_sizes),
        ]
        pad = MAX_OUTER_DIMS - len(it.outer_sizes)
        sizes = list(it.outer_sizes) + [1] * pad
        strides = list(it.outer_strides) + [0] * pad
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
        nbytes_list = [it.stored_bytes for it in items]
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
                        prev_end = it.flat_offset + it.stored_bytes
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
        stored_dtypes = _per_tensor_dtypes(stored_dtypes, len(tensors), "stored_dtypes")
        if not self._use_ext:
            return [
                torch_count_nonfinite(t, st)
                for t, st in zip(tensors, stored_dtypes)
            ]
        per_tensor, classes = build_scan_items(tensors, stored_dtypes)
        nans, infs = self._read_launch(
            # without a class there is nothing to count: (0, 0), no fallback
            [[] if cls is None else its for its, cls in zip(per_tensor, classes)],
            lambda items, owners, *where: _csnap.scan_nonfinite(
                _items_to_flat(items), [classes[i] for i in owners], len(items), *where
            ),
            2,
            lambda i: torch_count_nonfinite(tensors[i], stored_dtypes[i]),
        )
        return list(zip(nans, infs))

    # -- fingerprint --------------------------------------------------------

    def fingerprint(
        self,
        tensors: Sequence[torch.Tensor],
        stored_dtypes: Optional[Sequence[Optional[torch.dtype]]] = None,
        split_bytes: Optional[int] = None,
    ) -> List[int]:
        """psum64 of the bytes each of this device's ``tensors`` is stored
        as, from ONE read-only fingerprint-kernel launch over all of them:
        nothing is staged. Blocking.

        The value equals ``integrity.psum64_value`` of
        ``t.contiguous()``'s bytes (of ``t.to(stored).contiguous()``'s with
        ``stored_dtypes[i]`` bfloat16/float16 for a float32 tensor) and does
        not depend on the tensor's strides. It is a comparison of bytes:
        NaN payloads and the sign of zero count.

        Tensors build_fingerprint_items() declines are hashed on the host
        instead; so is everything when the extension is disabled by
        TSAMD_DISABLE_HIP_STAGING=1. ``split_bytes`` overrides the stored
        size from which a tensor is hashed in dim-0 pieces."""
        stored_dtypes = _per_tensor_dtypes(stored_dtypes, len(tensors), "stored_dtypes")
        if not self._use_ext:
            return [
                host_fingerprint(t, st) for t, st in zip(tensors, stored_dtypes)
            ]
        # descriptors state raw memory: lazy views are hashed by value, as
        # they are saved. The resolved copies live until the launch returns
        tensors = [
            t if t.is_quantized or t.layout != torch.strided else resolve_lazy(t)
            for t in tensors
        ]
        (sums,) = self._read_launch(
            build_fingerprint_items(tensors, stored_dtypes, split_bytes),
            lambda items, owners, *where: _csnap.fingerprint_tensors(
                _items_to_flat(items), len(items), *where
            ),
            1,
            lambda i: (host_fingerprint(tensors[i], stored_dtypes[i]),),
        )
        return sums

    # -- tensor statistics --------------------------------------------------

    def stats(
        self,
        tensors: Sequence[torch.Tensor],
        stored_dtypes: Optional[Sequence[Optional[torch.dtype]]] = None,
        max_grid: int = 0,
    ) -> List[List[int]]:
        """The six statistics words (decode_stats) of each of this device's
        ``tensors`` over its finite elements, from ONE read-only launch of
        the stats kernel over all of them. Blocking.

        Counts, minimum and maximum are exact. The sums are float64 and
        deterministic: the same tensor gives the same bits whatever else is
        in the batch and whatever ``max_grid`` (a bound on the kernel's
        workgroups, 0 = the extension's cap) says. The words of a tensor
        over the kernel's size cap are its dim-0 pieces' merged in order.
        Statistics are of the live values: ``stored_dtypes`` is accepted
        for state_checks.UniqueTensors.read and ignored. fp8, complex,
        integer, quantized and sparse tensors report STATS_EMPTY.

        Tensors build_stats_items() declines are computed with torch
        expressions instead; so is everything when the extension is
        disabled by TSAMD_DISABLE_HIP_STAGING=1."""
        if not self._use_ext:
            return [torch_tensor_stats(t) for t in tensors]
        per_tensor, classes = build_stats_items(tensors)
        columns = self._read_launch(
            # without a class there is nothing to report, and no fallback
            [[] if cls is None else its for its, cls in zip(per_tensor, classes)],
            lambda items, owners, stream, dev_index: _csnap.tensor_stats(
                _items_to_flat(items),
                len(items),
                [classes[i] for i in owners],
                dev_index,
                stream,
                max_grid,
            ),
            6,
            lambda i: torch_tensor_stats(tensors[i]),
            merge=merge_stats,
            empty=STATS_EMPTY,
        )
        return [list(row) for row in zip(*columns)] if tensors else []

    # -- exponent histograms --------------------------------------------------

    def hist(
        self,
        tensors: Sequence[torch.Tensor],
        stored_dtypes: Optional[Sequence[Optional[torch.dtype]]] = None,
        max_grid: int = 0,
    ) -> List[List[int]]:
        """The 280 histogram words (decode_hist) of each of this device's
        ``tensors``, from ONE read-only launch of the histogram kernel over
        all of them. Blocking.

        Every word is an exact count: the same tensor gives the same words
        whatever else is in the batch and whatever ``max_grid`` (a bound on
        the kernel's workgroups, 0 = the extension's cap) says. The words of
        a tensor over the kernel's size cap are the sums of its dim-0
        pieces'. The values are the live ones: ``stored_dtypes`` is accepted
        for state_checks.UniqueTensors.read and ignored. fp8, complex,
        integer, quantized and sparse tensors report zeros.

        Tensors build_stats_items() declines are computed with torch
        expressions instead; so is everything when the extension is
        disabled by TSAMD_DISABLE_HIP_STAGING=1."""
        if not self._use_ext:
            return [torch_tensor_hist(t) for t in tensors]
        per_tensor, classes = build_stats_items(tensors)
        columns = self._read_launch(
            # without a class there is nothing to report, and no fallback
            [[] if cls is None else its for its, cls in zip(per_tensor, classes)],
            lambda items, owners, stream, dev_index: _csnap.tensor_hist(
                _items_to_flat(items),
                len(items),
                [classes[i] for i in owners],
                dev_index,
                stream,
                max_grid,
            ),
            HIST_WORDS,
            lambda i: torch_tensor_hist(tensors[i]),
        )
        return [list(row) for row in zip(*columns)] if tensors else []

    # -- compare ------------------------------------------------------------

    def compare(
        self,
        flat: Any,
        nbytes: int,
        members: Sequence[Member],
    ) -> List[List[Any]]:
        """The six fields (torch_tensor_diff) of each member of one read:
        the first ``nbytes`` of ``flat`` against live tensors of this
        device, from ONE launch of the compare kernel (and its finish
        launch) over all eligible members. ``flat`` is the PinnedBlock the
        read landed in, which the kernel reads in place over PCIe, or a
        uint8 device tensor. ``members`` holds ``(live view, stored dtype,
        flat offset)`` triples. Nothing is written to either side, and no
        payload-sized device memory is allocated. Blocking.

        Members build_compare_items() declines are compared with the torch
        expression instead; so is everything when the extension is disabled
        by TSAMD_DISABLE_HIP_STAGING=1."""
        on_host = isinstance(flat, PinnedBlock)
        flat_u8 = flat.tensor if on_host else flat
        if self._use_ext:
            items, classes = build_compare_items(members, flat_u8.data_ptr())
        else:
            items = classes = [None] * len(members)
        out: List[Any] = [None] * len(members)
        taken = [i for i, it in enumerate(items) if it is not None]
        if taken:
            dev_index = self.device.index or 0
            with torch.cuda.device(dev_index):
                got = _csnap.compare_tensors(
                    _items_to_flat([items[i] for i in taken]),
                    len(taken),
                    [classes[i] for i in taken],
                    flat_u8.data_ptr(),
                    on_host,
                    nbytes,
                    torch.cuda.current_stream().cuda_stream,
                    dev_index,
                )
            for k, i in enumerate(taken):
                out[i] = decode_diff(got[6 * k : 6 * k + 6], classes[i])
        for i, (live, stored, off) in enumerate(members):
            if out[i] is None:
                piece = flat_u8[off : off + live.numel() * stored.itemsize]
                if (flat_u8.storage_offset() + off) % stored.itemsize:
                    piece = piece.clone()  # a view needs whole elements
                out[i] = torch_tensor_diff(
                    piece.view(stored).reshape(live.shape), live
                )
        return out

    # -- what the read-only launches share -----------------------------------

    def _read_launch(
        self,
        per_tensor: Sequence[Optional[List[PackItem]]],
        call: Callable[..., Sequence[int]],
        words: int,
        fallback: Callable[[int], Sequence[int]],
        merge: Optional[Callable[[Sequence[int], Sequence[int]], Sequence[int]]] = None,
        empty: Optional[Sequence[int]] = None,
    ) -> List[List[int]]:
        """``words`` u64 results for each tensor of a batch, from ONE
        extension call over every descriptor in ``per_tensor``; returned
        as one list per word, each with an entry per tensor.
        ``call(items, owners, stream, dev_index)`` makes the call and
        returns ``words`` values per descriptor; ``owners[k]`` is the index
        of the tensor that descriptor ``k`` belongs to. A None entry is a
        tensor the builder declined: ``fallback(index)`` answers for it.

        A tensor's descriptors are combined in one of two ways. Without
        ``merge`` its result is the sum of its descriptors' words mod 2^64
        (counts stay far below it), zeros without descriptors. With
        ``merge`` its result starts as ``empty`` and each descriptor's
        words, in order, are folded in as
        ``merge(so_far, words_of_descriptor)``."""
        items: List[PackItem] = []
        owners: List[int] = []
        for i, its in enumerate(per_tensor):
            for it in its or ():
                items.append(it)
                owners.append(i)
        out = [[e] * len(per_tensor) for e in (empty or [0] * words)]
        if items:
            dev_index = self.device.index or 0
            with torch.cuda.device(dev_index):
                got = call(
                    items, owners, torch.cuda.current_stream().cuda_stream, dev_index
                )
            if merge is None:
                for w, column in enumerate(out):
                    for i, v in zip(owners, got[w::words]):
                        column[i] = (column[i] + v) % (1 << 64)
            else:
                for k, i in enumerate(owners):
                    merged = merge(
                        [column[i] for column in out],
                        got[k * words : (k + 1) * words],
                    )
                    for column, v in zip(out, merged):
                        column[i] = v
        for i, its in enumerate(per_tensor):
            if its is None:
                for column, v in zip(out, fallback(i)):
                    column[i] = v
        return out

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
            if is_mx(out_dtype):
                flat = mx_encode_as(t, out_dtype)
            else:
                if it.cast != CAST_NONE:
                    t = t.to(out_dtype)
                flat = t.contiguous().reshape(-1).view(torch.uint8)
            dst = batch.pinned.tensor[
                it.flat_offset : it.flat_offset + it.stored_bytes
            ]
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
