"""Shared pieces of the non-finite scan tests: bit-pattern inputs per
element class, the CPU oracle (torch's own isnan/isinf, after ``.to(stored)``
for the two stored classes — never the code under test), and a Python
mirror of the kernel's classification table and descriptor walk."""

from typing import List, Optional, Tuple

import torch

from torchsnapshot_amd.ops import staging

_LOW_HALVES = [
    0x0000, 0x0001, 0x0FFF, 0x1000, 0x1001, 0x2FFF,
    0x3000, 0x3001, 0x7FFF, 0x8000, 0x8001, 0xFFFF,
]

# (id, dtype, stored dtype, scan class)
CLASSES = [
    ("f64", torch.float64, None, staging.SCAN_F64),
    ("f32", torch.float32, None, staging.SCAN_F32),
    ("f16", torch.float16, None, staging.SCAN_F16),
    ("bf16", torch.bfloat16, None, staging.SCAN_BF16),
    ("e5m2", torch.float8_e5m2, None, staging.SCAN_E5M2),
    ("e4m3fn", torch.float8_e4m3fn, None, staging.SCAN_E4M3FN),
    ("e4m3fnuz", torch.float8_e4m3fnuz, None, staging.SCAN_FNUZ),
    ("e5m2fnuz", torch.float8_e5m2fnuz, None, staging.SCAN_FNUZ),
    ("f32_as_f16", torch.float32, torch.float16, staging.SCAN_F32_AS_F16),
    ("f32_as_bf16", torch.float32, torch.bfloat16, staging.SCAN_F32_AS_BF16),
]
CLASS_IDS = [c[0] for c in CLASSES]

# totals over all patterns of the 1- and 2-byte dtypes, from torch's CPU
# isnan/isinf
EXPECTED_TOTALS = {
    "e4m3fn": (2, 0),
    "e5m2": (6, 2),
    "e4m3fnuz": (1, 0),
    "e5m2fnuz": (1, 0),
    "f16": (2046, 2),
    "bf16": (254, 2),
}

# the first float32 that narrows to f16 inf (65520.0) / bf16 inf, and their
# neighbours
THRESHOLD_NEIGHBOURS = [0x477FEFFF, 0x477FF000, 0x7F7F7FFF, 0x7F7F8000]

_F64_PATTERNS = [
    0x0000000000000000, 0x8000000000000000, 0x0000000000000001,
    0x3FF0000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,
    0x7FF0000000000000, 0xFFF0000000000000, 0x7FF0000000000001,
    0xFFF0000000000001, 0x7FF8000000000000, 0xFFFFFFFFFFFFFFFF,
    0x7FF00000FFFFFFFF, 0x7FEFFFFF00000000, 0x7FF0000100000000,
    0x000000007FF00000, 0x7FF0000000000000, 0x4000000000000000,
]


def bits_to_tensor(bits: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """int64 tensor of unsigned bit patterns (f64: already-signed int64) ->
    tensor of ``dtype`` with exactly those bits."""
    size = dtype.itemsize
    if size == 1:
        return bits.to(torch.uint8).view(dtype)
    if size == 2:
        signed = torch.where(bits >= 2**15, bits - 2**16, bits)
        return signed.to(torch.int16).view(dtype)
    if size == 4:
        signed = torch.where(bits >= 2**31, bits - 2**32, bits)
        return signed.to(torch.int32).view(dtype)
    return bits.view(dtype)


def _signed64(v: int) -> int:
    return v - 2**64 if v >= 2**63 else v


def all_patterns(dtype: torch.dtype) -> torch.Tensor:
    """Exhaustive inputs of a class: every pattern of a 1- or 2-byte dtype,
    every high half crossed with a dozen low halves (and the narrowing
    thresholds' neighbours, both signs) for float32, hand-picked patterns
    for float64."""
    size = dtype.itemsize
    if size == 1:
        bits = torch.arange(256, dtype=torch.int64)
    elif size == 2:
        bits = torch.arange(65536, dtype=torch.int64)
    elif size == 4:
        hi = torch.arange(65536, dtype=torch.int64).unsqueeze(1) << 16
        lo = torch.tensor(_LOW_HALVES, dtype=torch.int64).unsqueeze(0)
        near = torch.tensor(THRESHOLD_NEIGHBOURS, dtype=torch.int64)
        bits = torch.cat([(hi | lo).reshape(-1), near, near | 0x80000000])
    else:
        bits = torch.tensor(
            [_signed64(v) for v in _F64_PATTERNS], dtype=torch.int64
        )
    return bits_to_tensor(bits, dtype)


def oracle(
    t: torch.Tensor, stored: Optional[torch.dtype] = None
) -> Tuple[int, int]:
    """(NaN, Inf) counts by torch on the CPU."""
    c = t.detach().cpu()
    if c.dtype.is_complex:
        c = torch.view_as_real(c.resolve_conj())
    if stored is not None:
        c = c.to(stored)
    if c.dtype.itemsize == 1:
        c = c.to(torch.float32)
    return int(torch.isnan(c).sum()), int(torch.isinf(c).sum())


def to_bits(t: torch.Tensor) -> torch.Tensor:
    """Contiguous CPU float tensor -> int64 tensor of its bit patterns,
    unsigned except for float64 (two's complement int64)."""
    size = t.dtype.itemsize
    flat = t.reshape(-1)
    if size == 1:
        return flat.view(torch.uint8).to(torch.int64)
    if size == 2:
        return flat.view(torch.int16).to(torch.int64) & 0xFFFF
    if size == 4:
        return flat.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return flat.view(torch.int64)


def mirror_count(bits: torch.Tensor, cls: int) -> Tuple[int, int]:
    """The kernel's classification table on int64 bit patterns."""
    s = staging
    if cls == s.SCAN_F64:
        a = bits & 0x7FFFFFFFFFFFFFFF
        return int((a > 0x7FF0000000000000).sum()), int(
            (a == 0x7FF0000000000000).sum()
        )
    if cls in (s.SCAN_F32, s.SCAN_F32_AS_F16, s.SCAN_F32_AS_BF16):
        a = bits & 0x7FFFFFFF
        first_inf = {
            s.SCAN_F32: 0x7F800000,
            s.SCAN_F32_AS_F16: 0x477FF000,
            s.SCAN_F32_AS_BF16: 0x7F7F8000,
        }[cls]
        return int((a > 0x7F800000).sum()), int(
            ((a >= first_inf) & (a <= 0x7F800000)).sum()
        )
    if cls == s.SCAN_F16:
        a = bits & 0x7FFF
        return int((a > 0x7C00).sum()), int((a == 0x7C00).sum())
    if cls == s.SCAN_BF16:
        a = bits & 0x7FFF
        return int((a > 0x7F80).sum()), int((a == 0x7F80).sum())
    if cls == s.SCAN_E5M2:
        a = bits & 0x7F
        return int((a > 0x7C).sum()), int((a == 0x7C).sum())
    if cls == s.SCAN_E4M3FN:
        return int(((bits & 0x7F) == 0x7F).sum()), 0
    assert cls == s.SCAN_FNUZ
    return int((bits == 0x80).sum()), 0


def storage_bytes(t: torch.Tensor) -> torch.Tensor:
    """A CPU tensor's whole storage as a uint8 tensor."""
    storage = t.untyped_storage()
    u8 = torch.empty(storage.nbytes(), dtype=torch.uint8)
    u8.untyped_storage().copy_(storage)
    return u8


def walk_items(
    t: torch.Tensor, items: List[staging.PackItem], cls: int
) -> Tuple[int, int, int]:
    """Walk scan descriptors over a CPU tensor's storage the way the kernel
    does (row decomposition over the outer dims, one contiguous run per
    row): (elements visited, NaN, Inf) with the mirror classification."""
    u8 = storage_bytes(t)
    base0 = t.untyped_storage().data_ptr()
    real = torch.view_as_real(t) if t.dtype.is_complex else t
    esz = real.element_size()
    visited = nan = inf = 0
    for it in items:
        if it.nbytes == 0:
            continue
        assert it.vec >= esz and it.row_bytes % it.vec == 0
        assert it.src_ptr % it.vec == 0
        assert all(st % it.vec == 0 for st in it.outer_strides)
        rows = it.nbytes // it.row_bytes
        chunks = []
        for r in range(rows):
            off, rem = 0, r
            for k in reversed(range(len(it.outer_sizes))):
                off += (rem % it.outer_sizes[k]) * it.outer_strides[k]
                rem //= it.outer_sizes[k]
            src = it.src_ptr - base0 + off
            assert 0 <= src and src + it.row_bytes <= u8.numel()
            chunks.append(u8[src : src + it.row_bytes])
        raw = torch.cat(chunks).clone()
        bits = to_bits(raw.view(real.dtype))
        visited += bits.numel()
        n, i = mirror_count(bits, cls)
        nan += n
        inf += i
    return visited, nan, inf
