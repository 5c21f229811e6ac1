"""CPU mirror of the restore scatter kernel's address math, plus the host
logic that decides when the kernel may run.

``py_scatter`` reproduces, from the PackItem fields alone, what a scatter
descriptor makes the kernel do: flat-side (stored) byte positions walk the
rows starting at the item's explicit flat offset; a widen item writes
``2*vec`` target bytes at twice the within-row offset for every ``vec``
stored bytes. Run over a copy of the target's whole storage, its result
must equal what ``view.copy_(stored_values)`` leaves there, every byte
outside the view included."""

import pytest
import torch

from torchsnapshot_amd import knobs
from torchsnapshot_amd.io_preparers.sharded_tensor import (
    Overlap,
    contiguous_source_offset,
)
from torchsnapshot_amd.ops.staging import (
    CAST_BF16_TO_F32,
    CAST_F16_TO_F32,
    CAST_NONE,
    PackItem,
    _items_to_flat,
    _scatter_layout_plan,
    build_scatter_items,
    scatter_member,
    scatter_plan,
    widen_code,
)

from test_cast_layout import _FP32_CASES
from test_staging_layout import _CASES

_STORED = [torch.bfloat16, torch.float16]
_CODE = {torch.bfloat16: CAST_BF16_TO_F32, torch.float16: CAST_F16_TO_F32}
_STORED_OF_CODE = {v: k for k, v in _CODE.items()}

# "expanded" overlaps itself: not a scatter target (checked further down)
_WIDEN_CASES = [c for c in _FP32_CASES if c[0] != "expanded"]
_PLAIN_CASES = [c for c in _CASES if c[0] != "expanded"]

# a pretend address of the flat buffer and a payload offset inside it
_FLAT_BASE = 0x7F0000001000
_OFF = 768


def _storage_copy(t: torch.Tensor):
    """(flat tensor over a private copy of t's whole storage, t's view of it)."""
    st = t.untyped_storage()
    u8 = torch.empty(st.nbytes(), dtype=torch.uint8)
    u8.untyped_storage().copy_(st)
    full = u8.view(t.dtype)
    return full, torch.as_strided(full, t.shape, t.stride(), t.storage_offset())


def _widen(src: bytes, stored: torch.dtype) -> bytes:
    """The value conversion itself is torch's (the kernel's is checked
    bit-for-bit on the GPU); this file checks the addressing around it."""
    v = torch.frombuffer(bytearray(src), dtype=stored)
    return bytes(v.to(torch.float32).view(torch.uint8).numpy())


def py_scatter(t: torch.Tensor, it: PackItem, flat: bytes) -> bytes:
    """Built only from the PackItem fields (and the target's storage)."""
    full, _ = _storage_copy(t)
    out = bytearray(full.view(torch.uint8).numpy().tobytes())
    if it.nbytes == 0:
        return bytes(out)
    base = it.src_ptr - t.untyped_storage().data_ptr()
    rb, vec = it.row_bytes, it.vec
    scale = 1 if it.cast == CAST_NONE else 2
    for r in range(it.nbytes // rb):
        off = 0
        rem = r
        for k in reversed(range(len(it.outer_sizes))):
            idx = rem % it.outer_sizes[k]
            rem //= it.outer_sizes[k]
            off += idx * it.outer_strides[k]
        row_dst = base + off
        for i in range(0, rb, vec):  # one lane operation
            s = it.flat_offset + r * rb + i
            piece = flat[s : s + vec]
            if it.cast != CAST_NONE:
                piece = _widen(piece, _STORED_OF_CODE[it.cast])
            d = row_dst + scale * i
            out[d : d + scale * vec] = piece
    return bytes(out)


def _expected_storage(t: torch.Tensor, values: torch.Tensor) -> bytes:
    full, view = _storage_copy(t)
    view.copy_(values.reshape(view.shape))
    return full.view(torch.uint8).numpy().tobytes()


def _payload(values: torch.Tensor) -> bytes:
    """``values``' bytes at _OFF inside a buffer of 0xA5 filler."""
    c = values.contiguous().reshape(-1)
    body = c.view(torch.uint8).numpy().tobytes() if c.numel() else b""
    return b"\xa5" * _OFF + body + b"\xa5" * 64


@pytest.mark.parametrize("stored", _STORED, ids=["bf16", "f16"])
@pytest.mark.parametrize(
    "name,make", _WIDEN_CASES, ids=[c[0] for c in _WIDEN_CASES]
)
def test_widen_scatter_math_matches_torch(name, make, stored):
    torch.manual_seed(0)
    t = make()
    values = torch.randn(tuple(t.shape)).to(stored)
    it = build_scatter_items([t], [stored], [_OFF], flat_base=_FLAT_BASE)[0]
    assert py_scatter(t, it, _payload(values)) == _expected_storage(
        t, values.to(torch.float32)
    )
    if t.numel() == 0:
        assert it.nbytes == 0 and it.cast == CAST_NONE
        return
    assert it.cast == _CODE[stored]
    assert it.flat_offset == _OFF
    assert it.nbytes == t.numel() * 2
    assert it.vec in (16, 8, 4, 2)
    assert it.row_bytes % it.vec == 0 and it.nbytes % it.row_bytes == 0
    # tensor side: 2*vec bytes as one store, or two 16-byte stores at vec 16
    dst_align = min(16, 2 * it.vec)
    assert it.src_ptr % dst_align == 0
    assert all(st % dst_align == 0 for st in it.outer_strides)
    assert (_FLAT_BASE + it.flat_offset) % it.vec == 0


@pytest.mark.parametrize(
    "name,make", _PLAIN_CASES, ids=[c[0] for c in _PLAIN_CASES]
)
def test_plain_scatter_math_matches_torch(name, make):
    torch.manual_seed(0)
    t = make()
    values = (torch.rand(tuple(t.shape)) * 100).to(t.dtype)
    it = build_scatter_items([t], [t.dtype], [_OFF], flat_base=_FLAT_BASE)[0]
    assert it.cast == CAST_NONE and it.flat_offset == _OFF
    assert py_scatter(t, it, _payload(values)) == _expected_storage(t, values)
    assert (_FLAT_BASE + it.flat_offset) % it.vec == 0
    assert it.src_ptr % it.vec == 0


@pytest.mark.parametrize(
    "off,vec", [(0, 16), (256, 16), (8, 8), (4, 4), (6, 2), (2, 2)]
)
def test_vec_rule_includes_flat_address(off, vec):
    t = torch.zeros(64, 32)  # contiguous, 16-aligned: vec 16 on its own
    assert t.data_ptr() % 16 == 0
    it = build_scatter_items([t], [torch.bfloat16], [off], flat_base=4096)[0]
    assert it.vec == vec and it.flat_offset == off
    plain = build_scatter_items([t], [torch.float32], [off], flat_base=4096)[0]
    assert plain.vec == vec
    # it is the address that counts, not the offset: base 4098 is 2 mod 16
    it = build_scatter_items([t], [torch.bfloat16], [off], flat_base=4098)[0]
    assert it.vec == {0: 2, 256: 2, 8: 2, 4: 2, 6: 8, 2: 4}[off]


def test_odd_flat_address():
    t = torch.zeros(64, 32)
    with pytest.raises(ValueError, match="odd address"):
        build_scatter_items([t], [torch.bfloat16], [1], flat_base=4096)
    u8 = torch.zeros(100, dtype=torch.uint8)
    assert build_scatter_items([u8], [torch.uint8], [1], flat_base=4096)[0].vec == 1
    # an offset that splits an element is not a scatter member at all
    assert scatter_member(t, torch.bfloat16, 1) is None


def test_explicit_offsets_are_not_repacked():
    tensors = [torch.zeros(13, 7), torch.zeros(5), torch.zeros(3, 3).t()]
    stored = [torch.bfloat16, torch.float32, torch.float16]
    offsets = [4096, 10, 512]  # neither sorted nor 256-aligned
    items = build_scatter_items(tensors, stored, offsets, flat_base=1 << 20)
    assert [it.flat_offset for it in items] == offsets
    assert [it.cast for it in items] == [
        CAST_BF16_TO_F32, CAST_NONE, CAST_F16_TO_F32,
    ]
    assert items[1].vec == 2  # offset 10
    flat = _items_to_flat(items)
    assert len(flat) == 3 * 19
    assert [flat[i * 19 + 1] for i in range(3)] == offsets
    assert [flat[i * 19 + 18] for i in range(3)] == [3, 0, 4]


def test_widen_code_pairs():
    assert widen_code(torch.bfloat16, torch.float32) == CAST_BF16_TO_F32
    assert widen_code(torch.float16, torch.float32) == CAST_F16_TO_F32
    assert widen_code(torch.int64, torch.int64) == CAST_NONE
    for stored, target in [
        (torch.float32, torch.bfloat16),
        (torch.bfloat16, torch.float16),
        (torch.float16, torch.float64),
        (torch.int8, torch.float32),
    ]:
        with pytest.raises(ValueError):
            widen_code(stored, target)


# ---------------------------------------------------------------------------
# eligibility. scatter_plan() declines every non-CUDA target first; the
# layout classes behind that check are asked of _scatter_layout_plan, which
# is scatter_plan() past the device test.
# ---------------------------------------------------------------------------


def test_plan_declines_host_targets():
    assert scatter_plan(torch.zeros(4, 4), torch.float32) is None
    assert scatter_plan(torch.empty(4, device="meta"), torch.float32) is None
    assert scatter_member(torch.zeros(4, 4), torch.float32, 0) is None


def test_plan_accepts_plain_layouts():
    assert _scatter_layout_plan(torch.zeros(4, 4), torch.float32) == CAST_NONE
    assert _scatter_layout_plan(torch.zeros(4, 4), torch.bfloat16) == CAST_BF16_TO_F32
    assert _scatter_layout_plan(torch.zeros(4, 4).t(), torch.float16) == CAST_F16_TO_F32
    assert _scatter_layout_plan(torch.tensor(1.0), torch.bfloat16) == CAST_BF16_TO_F32
    assert _scatter_layout_plan(torch.zeros(9, 4)[2:6], torch.float32) == CAST_NONE


def _misaligned_f32() -> torch.Tensor:
    t = torch.frombuffer(bytearray(64), dtype=torch.float32, count=8, offset=1)
    if t.data_ptr() % 4 == 0:  # the bytearray itself sat at an odd address
        t = torch.frombuffer(bytearray(64), dtype=torch.float32, count=8, offset=2)
    assert t.data_ptr() % 4 != 0
    return t


_INELIGIBLE = [
    ("sparse", lambda: torch.zeros(4, 4).to_sparse(), torch.float32),
    (
        "quantized",
        lambda: torch.quantize_per_tensor(torch.zeros(4), 0.1, 0, torch.qint8),
        torch.qint8,
    ),
    ("stride-0", lambda: torch.zeros(1, 16).expand(8, 16), torch.float32),
    (
        "overlapping-rows",
        lambda: torch.as_strided(torch.zeros(16), (4, 4), (2, 1)),
        torch.float32,
    ),
    # dense, so torch rules overlap out; nothing merges: 8 outer dims
    (
        "8-outer-dims",
        lambda: torch.zeros([2] * 8).permute(7, 6, 5, 4, 3, 2, 1, 0),
        torch.float32,
    ),
    ("narrowing-pair", lambda: torch.zeros(4, dtype=torch.bfloat16), torch.float32),
    ("f16-to-bf16", lambda: torch.zeros(4, dtype=torch.bfloat16), torch.float16),
    ("int-to-float", lambda: torch.zeros(4), torch.int32),
    ("8GiB", lambda: torch.empty(2**31, device="meta"), torch.float32),
    ("4GiB-stored", lambda: torch.empty(2**31, device="meta"), torch.bfloat16),
    ("misaligned-elements", _misaligned_f32, torch.float32),
]


@pytest.mark.parametrize(
    "name,make,stored", _INELIGIBLE, ids=[c[0] for c in _INELIGIBLE]
)
def test_plan_declines_each_ineligible_class(name, make, stored):
    assert _scatter_layout_plan(make(), stored) is None


def test_plan_size_limit_is_just_under_4gib():
    ok = torch.empty(2**31 - 2**15 - 8, device="meta")
    assert _scatter_layout_plan(ok, torch.bfloat16) == CAST_BF16_TO_F32


# ---------------------------------------------------------------------------
# ShardConsumer's contiguous-source predicate
# ---------------------------------------------------------------------------


def _ov(src_offsets, lengths):
    return Overlap(
        src_offsets=list(src_offsets),
        dst_offsets=[0] * len(lengths),
        lengths=list(lengths),
    )


def test_row_split_is_a_contiguous_source():
    shape = (90, 66)
    assert contiguous_source_offset(shape, _ov([0, 0], [90, 66])) == 0
    assert contiguous_source_offset(shape, _ov([45, 0], [15, 66])) == 45 * 66
    # part of a single row is one run as well
    assert contiguous_source_offset(shape, _ov([7, 22], [1, 11])) == 7 * 66 + 22


def test_column_split_is_not():
    shape = (90, 66)
    assert contiguous_source_offset(shape, _ov([0, 22], [90, 11])) is None
    assert contiguous_source_offset(shape, _ov([10, 0], [20, 65])) is None
    assert contiguous_source_offset((4, 5, 6), _ov([1, 0, 0], [2, 5, 6])) == 30
    assert contiguous_source_offset((4, 5, 6), _ov([0, 1, 0], [4, 2, 6])) is None


# ---------------------------------------------------------------------------
# knob
# ---------------------------------------------------------------------------


def test_restore_mode_knob(monkeypatch):
    monkeypatch.delenv("TSAMD_RESTORE_MODE", raising=False)
    assert knobs.get_restore_mode() == "torch"  # see docs/design.md, Restore
    for mode in ("direct", "slab", "torch"):
        monkeypatch.setenv("TSAMD_RESTORE_MODE", mode)
        assert knobs.get_restore_mode() == mode
    monkeypatch.setenv("TSAMD_RESTORE_MODE", "sdma")
    with pytest.raises(ValueError, match="TSAMD_RESTORE_MODE"):
        knobs.get_restore_mode()
    # "torch" switches the kernel path off for every target
    monkeypatch.setenv("TSAMD_RESTORE_MODE", "torch")
    assert scatter_member(torch.zeros(4), torch.float32, 0) is None
