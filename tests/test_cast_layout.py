"""CPU mirror of the gather-and-cast kernel's address math.

``py_cast_pack`` reproduces, from the PackItem fields alone, what a cast
descriptor makes the kernel do: flat-side (stored) byte positions walk the
rows, the source sits at twice the within-row offset, and every lane
operation converts ``vec`` stored bytes from ``2*vec`` source bytes. Its
output must equal ``t.contiguous().to(dst)``'s bytes for every fp32 layout
of test_staging_layout's ``_CASES``."""

import pytest
import torch

from torchsnapshot_amd.ops.staging import (
    ALIGN,
    CAST_F32_TO_BF16,
    CAST_F32_TO_F16,
    CAST_NONE,
    PackItem,
    _items_to_flat,
    build_pack_items,
)

from test_staging_layout import _CASES

_TARGETS = [torch.bfloat16, torch.float16]
_CODE = {torch.bfloat16: CAST_F32_TO_BF16, torch.float16: CAST_F32_TO_F16}
_DST_OF_CODE = {v: k for k, v in _CODE.items()}

_FP32_CASES = [c for c in _CASES if c[1]().dtype == torch.float32]
# plus the layouts the cast GPU tests use, scaled down
_FP32_CASES += [
    ("odd-wide-tail", lambda: torch.randn(6, 1100)[:, :1030]),
    ("three-elem-rows", lambda: torch.randn(50, 8)[:, :3]),
    ("misaligned-base", lambda: torch.randn(1001).view(-1)[1:]),
    ("base+8", lambda: torch.randn(1002)[2:]),
    ("empty", lambda: torch.empty(0, 4)),
]


def _storage_bytes(t: torch.Tensor) -> bytes:
    storage = t.untyped_storage()
    u8 = torch.empty(storage.nbytes(), dtype=torch.uint8)
    u8.untyped_storage().copy_(storage)
    return bytes(u8.numpy())


def _convert(src: bytes, dst: torch.dtype) -> bytes:
    """The value conversion itself is torch's (the kernel's is checked
    bit-for-bit on the GPU); this file checks the addressing around it."""
    f = torch.frombuffer(bytearray(src), dtype=torch.float32)
    return bytes(f.to(dst).view(torch.uint8).numpy())


def py_cast_pack(t: torch.Tensor, it: PackItem) -> bytes:
    """Built only from the PackItem fields (and the tensor's storage)."""
    if it.nbytes == 0:
        return b""
    assert it.cast in _DST_OF_CODE
    dst = _DST_OF_CODE[it.cast]
    storage_b = _storage_bytes(t)
    base = it.src_ptr - t.untyped_storage().data_ptr()
    rb, vec = it.row_bytes, it.vec
    out = bytearray(it.nbytes)
    for r in range(it.nbytes // rb):
        off = 0
        rem = r
        for k in reversed(range(len(it.outer_sizes))):
            idx = rem % it.outer_sizes[k]
            rem //= it.outer_sizes[k]
            off += idx * it.outer_strides[k]
        row_src = base + off
        for i in range(0, rb, vec):  # one lane operation
            s = row_src + 2 * i
            out[r * rb + i : r * rb + i + vec] = _convert(
                storage_b[s : s + 2 * vec], dst
            )
    return bytes(out)


def _ref_bytes(t: torch.Tensor, dst: torch.dtype) -> bytes:
    c = t.contiguous().to(dst).reshape(-1)
    if c.numel() == 0:
        return b""
    return bytes(c.view(torch.uint8).numpy())


@pytest.mark.parametrize("dst", _TARGETS, ids=["bf16", "f16"])
@pytest.mark.parametrize(
    "name,make", _FP32_CASES, ids=[c[0] for c in _FP32_CASES]
)
def test_cast_pack_math_matches_torch(name, make, dst):
    torch.manual_seed(0)
    t = make()
    items, offsets, total = build_pack_items([t], [dst])
    it = items[0]
    assert py_cast_pack(t, it) == _ref_bytes(t, dst)
    assert it.nbytes == t.numel() * 2
    assert offsets == [0]
    assert total == (it.nbytes + ALIGN - 1) // ALIGN * ALIGN


@pytest.mark.parametrize("dst", _TARGETS, ids=["bf16", "f16"])
@pytest.mark.parametrize(
    "name,make", _FP32_CASES, ids=[c[0] for c in _FP32_CASES]
)
def test_cast_vec_alignment(name, make, dst):
    t = make()
    items, _, _ = build_pack_items([t], [dst])
    it = items[0]
    if it.nbytes == 0:
        assert it.cast == CAST_NONE
        return
    assert it.cast == _CODE[dst]
    assert it.vec in (16, 8, 4, 2)
    assert it.row_bytes % it.vec == 0
    assert it.nbytes % it.row_bytes == 0
    # every vector load is naturally aligned: 2*vec source bytes are read
    # as one load of that width, or as two 16-byte loads at vec == 16
    src_align = min(16, 2 * it.vec)
    assert it.src_ptr % src_align == 0
    for st in it.outer_strides:
        assert st % src_align == 0
    # flat side: 256-aligned base + multiples of vec
    assert it.flat_offset % ALIGN == 0


def test_misaligned_base_takes_narrowest_vector():
    t = torch.randn(1001)[1:]  # base is 4 mod 8
    if t.data_ptr() % 8 == 0:
        t = torch.randn(1002)[2:][1:]
    assert t.data_ptr() % 8 == 4
    items, _, _ = build_pack_items([t], [torch.bfloat16])
    assert items[0].vec == 2


def test_interleaved_cast_uncast_offsets_use_stored_sizes():
    tensors = [
        torch.randn(13, 7),                       # cast
        torch.randn(13, 7),                       # uncast fp32
        torch.arange(10, dtype=torch.int64),      # uncast
        torch.randn(5, 3).t(),                    # cast, strided
        torch.randn(9).to(torch.bfloat16),        # bf16 source, as is
        torch.empty(0),                           # empty, cast requested
        torch.randn(300),                         # cast
    ]
    outs = [
        torch.bfloat16, None, None, torch.float16, torch.bfloat16,
        torch.float16, torch.float16,
    ]
    items, offsets, total = build_pack_items(tensors, outs)
    stored = [
        t.numel() * (2 if (o is not None and t.dtype == torch.float32)
                     else t.element_size())
        for t, o in zip(tensors, outs)
    ]
    expect_off = 0
    for it, off, n in zip(items, offsets, stored):
        assert off % ALIGN == 0
        assert off == expect_off == it.flat_offset
        assert it.nbytes == n
        expect_off += (n + ALIGN - 1) // ALIGN * ALIGN
    assert total == expect_off
    codes = [it.cast for it in items]
    assert codes == [
        CAST_F32_TO_BF16, CAST_NONE, CAST_NONE, CAST_F32_TO_F16, CAST_NONE,
        CAST_NONE, CAST_F32_TO_F16,
    ]
    # uncast members are described exactly as without out_dtypes
    plain, _, _ = build_pack_items([tensors[1]])
    assert items[1].vec == plain[0].vec
    assert items[1].row_bytes == plain[0].row_bytes


def test_descriptor_row_carries_cast_code():
    t = torch.randn(4, 4)
    items, _, _ = build_pack_items([t, t], [torch.float16, None])
    flat = _items_to_flat(items)
    assert len(flat) == 2 * 19
    assert flat[18] == CAST_F32_TO_F16
    assert flat[19 + 18] == CAST_NONE


@pytest.mark.parametrize(
    "src,dst",
    [
        (torch.float32, torch.int8),
        (torch.float32, torch.float64),
        (torch.float64, torch.bfloat16),
        (torch.bfloat16, torch.float16),
        (torch.int64, torch.float16),
    ],
)
def test_unsupported_pair_raises(src, dst):
    t = torch.zeros(8, dtype=src)
    with pytest.raises(ValueError):
        build_pack_items([t], [dst])
