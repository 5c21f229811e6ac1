"""Shared layout table of the staging-kernel sweep (not a conftest).

A *recipe* is plain data: dtype, base shape, storage offset in elements,
per-dim slices, expanded dims, a permutation and an optional lazy bit.
``make(recipe, device)`` cuts the view it describes out of a 1-D storage
tensor that is longer than the view on both sides and holds distinct,
position-dependent bit patterns, so that a misplaced element shows and so
does a write outside the view. The storage's address is asserted to be
16-aligned on whichever device it is built on: a descriptor's vec then
depends on the recipe alone, and descriptors built from the CPU view and
from a device view agree in every field but ``src_ptr``.

``FIXED`` is the hand-made table whose coverage the CPU tests assert cell by
cell; ``RANDOM`` is a seeded extension (``random.Random``, no hypothesis:
the same recipes in every run and on every machine).

Also here: ``py_pack``, the Python mirror of the gather kernel's address
arithmetic, and the classification helpers the CPU and GPU modules share.
"""

import math
import random
from dataclasses import dataclass
from typing import Callable, List, Optional, Tuple

import torch

from torchsnapshot_amd.ops import staging
from torchsnapshot_amd.ops.staging import build_pack_items

# elements of storage in front of (and at least behind) every base tensor.
# 16 elements are a multiple of 16 bytes for every dtype, so the pad does
# not change any alignment.
PAD = 16
WORK_UNIT = 64 * 1024
WIDE_ROW = 2048
MAX_PAYLOAD = 200 * 1024

DTYPES = [
    torch.uint8,
    torch.bfloat16,
    torch.float32,
    torch.float64,
    torch.complex128,
]


@dataclass(frozen=True)
class Recipe:
    name: str
    dtype: torch.dtype
    shape: Tuple[int, ...]  # base tensor, contiguous in the storage
    offset: int = 0  # storage offset in elements, on top of PAD
    # per base dim (start, stop, step); stop None = to the end
    slices: Optional[Tuple[Tuple[int, Optional[int], int], ...]] = None
    # (dim, size): expand that size-1 dim (after slicing, before permuting)
    expand: Tuple[Tuple[int, int], ...] = ()
    perm: Optional[Tuple[int, ...]] = None
    lazy: str = ""  # "", "conj" or "neg"
    # what the table says the kernel paths must decline: any of
    # "stride0", "dims" (more than 6 outer dims), "lazy"
    declines: Tuple[str, ...] = ()


def _mixed_ramp(n: int) -> torch.Tensor:
    """int64 values that differ from element to element in every byte."""
    i = torch.arange(1, n + 1, dtype=torch.int64)
    v = i * -7046029254386353131  # 0x9E3779B97F4A7C15 as int64; wraps
    return v ^ (v >> 29)


def ramp_fill(dtype: torch.dtype, n: int) -> torch.Tensor:
    """1-D CPU tensor of ``n`` elements: an integer ramp, mixed so that no
    byte repeats with a short period, reinterpreted as ``dtype``."""
    esz = dtype.itemsize
    if esz == 16:
        return _mixed_ramp(2 * n).view(torch.float64).view(dtype)
    ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[esz]
    return _mixed_ramp(n).to(ints).view(dtype)


def byte_fill(value: int) -> Callable[[torch.dtype, int], torch.Tensor]:
    def fill(dtype: torch.dtype, n: int) -> torch.Tensor:
        return torch.full((n * dtype.itemsize,), value, dtype=torch.uint8).view(
            dtype
        )

    return fill


def value_fill(dtype: torch.dtype, n: int) -> torch.Tensor:
    """Position-dependent finite values (no NaN patterns), for comparisons
    by value such as ``check_state_dict_eq``."""
    i = torch.arange(n, dtype=torch.int64)
    if dtype == torch.uint8:
        return ((i % 251) + 3 * (i // 251)).to(torch.uint8)
    x = ((i % 2039) - 1000).to(torch.float64) * 0.25 + (i // 2039).to(torch.float64)
    if dtype.is_complex:
        return torch.complex(x, 0.5 - x / 2).to(dtype)
    return x.to(dtype)


def cast_fill(dtype: torch.dtype, n: int) -> torch.Tensor:
    """float32 values for the cast and widen sweeps: finite, normal in
    float16 and bfloat16 after rounding, plus +-0 and +-inf."""
    assert dtype == torch.float32
    i = torch.arange(n, dtype=torch.int64)
    mant = 1.0 + (i % 1009).to(torch.float64) / 1009.0
    x = mant * torch.pow(2.0, ((i % 21) - 10).to(torch.float64))
    x = torch.where(i % 2 == 1, -x, x).to(torch.float32)
    specials = torch.tensor([0.0, -0.0, float("inf"), float("-inf")])
    pick = i % 13 == 5
    x[pick] = specials[(i[pick] // 13) % 4]
    return x


def storage_numel(r: Recipe) -> int:
    return PAD + r.offset + math.prod(r.shape) + PAD


def cut(r: Recipe, storage: torch.Tensor) -> torch.Tensor:
    """The recipe's view of ``storage`` (1-D, ``r.dtype``, any device)."""
    assert storage.dim() == 1 and storage.dtype == r.dtype
    assert storage.numel() == storage_numel(r)
    assert storage.data_ptr() % 16 == 0, "storage must be 16-aligned"
    start = PAD + r.offset
    v = storage[start : start + math.prod(r.shape)].view(r.shape)
    if r.slices is not None:
        assert len(r.slices) == len(r.shape)
        v = v[tuple(slice(a, b, c) for a, b, c in r.slices)]
    if r.expand:
        sizes = list(v.shape)
        for dim, size in r.expand:
            assert sizes[dim] == 1
            sizes[dim] = size
        v = v.expand(sizes)
    if r.perm is not None:
        v = v.permute(r.perm)
    if r.lazy == "conj":
        v = v.conj()
        assert v.is_conj()
    elif r.lazy == "neg":
        v = torch._neg_view(v)
        assert v.is_neg()
    return v


def make(
    r: Recipe,
    device="cpu",
    fill: Callable[[torch.dtype, int], torch.Tensor] = ramp_fill,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """(storage, view) of a recipe on ``device``. The storage is filled on
    the CPU and copied over, so every device sees the same bytes."""
    storage = fill(r.dtype, storage_numel(r))
    assert storage.device.type == "cpu" and storage.numel() == storage_numel(r)
    if torch.device(device).type != "cpu":
        storage = storage.to(device)
    return storage, cut(r, storage)


def resolved(view: torch.Tensor) -> torch.Tensor:
    """The values a view stands for: lazy conj/neg bits applied."""
    return view.resolve_conj().resolve_neg()


def raw_bytes(t: torch.Tensor) -> bytes:
    """Bytes of a whole contiguous tensor (any device), bit for bit."""
    c = t.detach().cpu().contiguous().reshape(-1)
    if c.numel() == 0:
        return b""
    return bytes(c.view(torch.uint8).numpy())


def ref_bytes(t: torch.Tensor) -> bytes:
    """What a snapshot must hold for ``t``: ``contiguous()`` bytes of the
    resolved values."""
    return raw_bytes(resolved(t.detach().cpu()))


# ---------------------------------------------------------------------------
# Python mirror of the gather kernel's address arithmetic
# ---------------------------------------------------------------------------


def py_pack(t: torch.Tensor) -> bytes:
    """Gather ``t``'s bytes the way the pack kernel does from its PackItem:
    row decomposition over the outer dims, one contiguous run per row."""
    items, _, _ = build_pack_items([t])
    it = items[0]
    if it.nbytes == 0:
        return b""
    storage = t.untyped_storage()
    # read the storage bytes directly
    u8 = torch.empty(storage.nbytes(), dtype=torch.uint8)
    u8.untyped_storage().copy_(storage)
    storage_b = bytes(u8.numpy())
    base = t.data_ptr() - storage.data_ptr()
    rb = it.row_bytes
    out = bytearray(it.nbytes)
    rows = it.nbytes // rb
    for r in range(rows):
        off = 0
        rem = r
        for k in reversed(range(len(it.outer_sizes))):
            idx = rem % it.outer_sizes[k]
            rem //= it.outer_sizes[k]
            off += idx * it.outer_strides[k]
        src = base + off
        out[r * rb : (r + 1) * rb] = storage_b[src : src + rb]
    return bytes(out)


# ---------------------------------------------------------------------------
# classification
# ---------------------------------------------------------------------------


def traversal_of(it: staging.PackItem) -> str:
    """Which branch of the kernels' traversal a descriptor takes."""
    if not it.outer_sizes or it.row_bytes == it.nbytes:
        return "contiguous"
    return "wide" if it.row_bytes >= WIDE_ROW else "narrow"


def size_class(nbytes: int) -> str:
    return "big" if nbytes > WORK_UNIT else "small"


def outer_dims(view: torch.Tensor) -> int:
    """Strided dims the kernels have to decompose, counted without the
    builders: runs of logically adjacent, jointly contiguous dims count
    once, and an innermost run of stride 1 is the row itself."""
    dims = [(s, st) for s, st in zip(view.shape, view.stride()) if s != 1]
    if not dims:
        return 0
    runs = 1
    for (_, st_out), (s_in, st_in) in zip(dims, dims[1:]):
        if st_out != s_in * st_in:
            runs += 1
    return runs - 1 if dims[-1][1] == 1 else runs


def scan_outer_dims(view: torch.Tensor) -> int:
    """outer_dims() for the scan, which does not care about element order:
    dims sorted by stride (expanded ones outermost) before runs are
    counted, complex tensors as their real components."""
    if view.dtype.is_complex:
        view = torch.view_as_real(view.conj() if view.is_conj() else view)
    dims = [(st, s) for s, st in zip(view.shape, view.stride()) if s != 1]
    if not dims:
        return 0
    dims = [d for d in dims if d[0] == 0] + sorted(
        (d for d in dims if d[0] != 0), reverse=True
    )
    runs = 1
    for (st_out, _), (st_in, s_in) in zip(dims, dims[1:]):
        if st_out != s_in * st_in:
            runs += 1
    return runs - 1 if dims[-1][0] == 1 else runs


def has_stride0(view: torch.Tensor) -> bool:
    return any(st == 0 and s > 1 for s, st in zip(view.shape, view.stride()))


def is_dense(view: torch.Tensor) -> bool:
    """Non-overlapping and dense: the elements fill one gap-free span."""
    if view.numel() == 0:
        return True
    dims = sorted(
        (st, s) for s, st in zip(view.shape, view.stride()) if s != 1
    )
    expect = 1
    for st, s in dims:
        if st != expect:
            return False
        expect *= s
    return True


def expected_declines(r: Recipe, view: torch.Tensor) -> Tuple[str, ...]:
    """The decline marks a recipe should carry, from torch-level facts."""
    out = []
    if has_stride0(view):
        out.append("stride0")
    if outer_dims(view) > 6:
        out.append("dims")
    if r.lazy:
        out.append("lazy")
    return tuple(out)


def kernel_scatter_ok(r: Recipe) -> bool:
    """The scatter kernel can write this view: no element is written twice
    (the views are cut by slicing, permuting and expanding only, so
    stride 0 is the one way to overlap), at most 6 outer dims, no lazy bit."""
    return not r.declines


def payload_bytes(r: Recipe) -> int:
    view = cut(r, torch.empty(storage_numel(r), dtype=r.dtype))
    return view.numel() * view.element_size()


def scatter_flat_offsets(recipes, stored_esz):
    """Flat offsets of the scatter sweep: member ``k`` at
    ``256*k + j*esz`` with ``j`` cycling through ``0 .. 16/esz - 1``, so
    the flat address limits vec as well."""
    offs, slot, j_of = [], 0, {}
    for r, esz in zip(recipes, stored_esz):
        nbytes = payload_bytes(r) // r.dtype.itemsize * esz
        j = j_of.get(esz, 0) % (16 // esz)
        j_of[esz] = j_of.get(esz, 0) + 1
        offs.append(256 * slot + j * esz)
        slot += (j * esz + nbytes + 255) // 256 + 1
    return offs


# ---------------------------------------------------------------------------
# the fixed table
# ---------------------------------------------------------------------------

u8, bf16, f32, f64, c128 = DTYPES
c64 = torch.complex64
_ALL = (0, None, 1)


def _cols(n: int, start: int = 0):
    """Slice spec of a 2-D base: all rows, columns [start, start + n)."""
    return (_ALL, (start, start + n, 1))


def _rev(n: int) -> Tuple[int, ...]:
    return tuple(reversed(range(n)))


FIXED: List[Recipe] = [
    # -- contiguous, vec 16/8/4/2/1: small and just over one work unit ------
    Recipe("contig-v16", f32, (8, 12)),
    Recipe("contig-v16-big", f32, (4100, 4)),
    Recipe("contig-v16-12", f32, (12,)),
    Recipe("contig-v8", f64, (9,), offset=1),
    Recipe("contig-v8-big", f64, (8201,), offset=1),
    Recipe("contig-v8-f32", f32, (30,), offset=2),
    Recipe("contig-v4", f32, (25,), offset=1),
    Recipe("contig-v4-big", f32, (16411,), offset=1),
    Recipe("contig-v2", bf16, (37,), offset=1),
    Recipe("contig-v2-big", bf16, (32801,), offset=1),
    Recipe("contig-v1", u8, (99,), offset=1),
    Recipe("contig-v1-big", u8, (65601,), offset=3),
    Recipe("contig-v1-oddcount", u8, (97,)),
    # -- wide rows (>= 2048 B): a 64 KiB cut falls inside a row -------------
    Recipe("wide-v16", f32, (2, 1200), slices=_cols(1032)),
    Recipe("wide-v16-big", f32, (17, 1200), slices=_cols(1032)),
    Recipe("wide-v16-1028", f32, (2, 1200), slices=_cols(1028)),
    Recipe("wide-v8", f64, (2, 300), slices=_cols(257)),
    Recipe("wide-v8-big", f64, (33, 300), slices=_cols(257)),
    Recipe("wide-v8-f32", f32, (2, 1200), slices=_cols(1026)),
    Recipe("wide-v4", f32, (2, 1200), slices=_cols(1025)),
    Recipe("wide-v4-big", f32, (17, 1200), slices=_cols(1025)),
    Recipe("wide-v2", bf16, (2, 1030), offset=1, slices=_cols(1025)),
    Recipe("wide-v2-big", bf16, (40, 1030), offset=1, slices=_cols(1025)),
    Recipe("wide-v1", u8, (2, 2100), slices=_cols(2049)),
    Recipe("wide-v1-big", u8, (33, 2100), slices=_cols(2049, start=1)),
    Recipe("wide-v16-c128", c128, (3, 150), slices=_cols(129, start=2)),
    # -- narrow rows --------------------------------------------------------
    Recipe("narrow-v16", f32, (9, 12), slices=_cols(8)),
    Recipe("narrow-v16-big", c128, (5000, 2), slices=(_ALL, (0, 1, 1))),
    Recipe("narrow-v16-c128", c128, (6, 2), slices=(_ALL, (1, 2, 1))),
    Recipe("narrow-v8", f64, (7, 3), slices=_cols(1)),
    Recipe("narrow-v8-big", f64, (9000, 3), slices=_cols(1)),
    Recipe("narrow-v8-f32", f32, (11, 12), slices=_cols(4, start=4)),
    Recipe("narrow-v8-f32-6", f32, (13, 6), slices=_cols(2)),
    Recipe("narrow-v4", f32, (10, 7), slices=_cols(3)),
    Recipe("narrow-v4-big", f32, (5500, 7), slices=_cols(3, start=2)),
    Recipe("narrow-v2", bf16, (12, 9), slices=_cols(5)),
    Recipe("narrow-v2-big", bf16, (6600, 9), slices=_cols(5, start=1)),
    Recipe("narrow-v1", u8, (14, 11), slices=_cols(7)),
    Recipe("narrow-v1-big", u8, (9400, 11), slices=_cols(7, start=3)),
    # innermost stride != 1: rows of one element, 8- and 16-byte elements
    Recipe("step2-f64", f64, (50,), slices=((1, None, 2),)),
    Recipe("step3-c128", c128, (40,), slices=((0, None, 3),)),
    # -- outer-dim counts 2..6 (1 is every 2-D slice above), then 7 and 8 ---
    Recipe("outer2", f32, (5, 6, 8), slices=(_ALL, (0, None, 2), (0, 6, 1))),
    Recipe("outer3", bf16, (3, 4, 5), perm=_rev(3)),
    Recipe(
        "outer4",
        f64,
        (3, 4, 5, 6),
        slices=((0, None, 2), (1, None, 2), (0, None, 2), (0, 4, 1)),
        perm=(2, 0, 3, 1),
    ),
    Recipe("outer5", u8, (2, 3, 2, 3, 4), perm=_rev(5)),
    Recipe("outer6", f32, (2, 3, 2, 3, 2, 3), perm=_rev(6)),
    Recipe("outer6-rows", c128, (3, 2, 3, 2, 3, 2, 4),
           slices=((0, None, 2),) * 6 + ((1, 3, 1),)),
    Recipe("outer7", f32, (2, 3, 2, 2, 3, 2, 2), perm=_rev(7), declines=("dims",)),
    Recipe("outer8", bf16, (2,) * 8, perm=_rev(8), declines=("dims",)),
    # gaps in every dim: these stay 7 and 8 dims even sorted by stride, as
    # the scan sorts them
    Recipe("outer7-gaps", f64, (3,) * 7, slices=((0, None, 2),) * 7,
           declines=("dims",)),
    Recipe("outer8-gaps", f32, (3,) * 8, slices=((0, None, 2),) * 8,
           perm=(1, 0, 3, 2, 5, 4, 7, 6), declines=("dims",)),
    # -- special layouts ----------------------------------------------------
    Recipe("stride0-outer", f32, (1, 16), expand=((0, 8),), declines=("stride0",)),
    Recipe("stride0-middle", f64, (4, 1, 6), expand=((1, 5),), declines=("stride0",)),
    Recipe("stride0-inner", bf16, (6, 1), expand=((1, 4),), declines=("stride0",)),
    Recipe("stride0-big", f32, (1, 130), expand=((0, 127),), declines=("stride0",)),
    Recipe("size1-dims", f32, (4, 1, 8, 1)),
    Recipe("size1-dims-t", f32, (4, 1, 8, 1), perm=(2, 1, 0, 3)),
    Recipe("scalar", f32, ()),
    Recipe("scalar-c128", c128, (), offset=3),
    Recipe("empty", f32, (0,)),
    Recipe("empty-3d", bf16, (3, 0, 2)),
    # -- lazy views ---------------------------------------------------------
    Recipe("conj", c64, (6, 10), lazy="conj", declines=("lazy",)),
    Recipe("conj-t", c64, (6, 10), perm=(1, 0), lazy="conj", declines=("lazy",)),
    Recipe("neg", f32, (7, 9), lazy="neg", declines=("lazy",)),
]


# ---------------------------------------------------------------------------
# the seeded random extension
# ---------------------------------------------------------------------------

_SEED = 20240611
_N_RANDOM = 100
_MAX_STORAGE = 1 << 20


def _random_recipe(rng: random.Random, k: int) -> Recipe:
    dtype = rng.choice(DTYPES)
    esz = dtype.itemsize
    ndim = rng.randint(1, 8)
    sizes = [rng.randint(1, 9) for _ in range(ndim)]
    # most members stay tiny
    while math.prod(sizes) * esz > 4096:
        sizes[sizes.index(max(sizes))] -= 1
    if rng.random() < 0.15:
        # stretch one dim so the payload passes one work unit
        d = rng.randrange(ndim)
        rest = math.prod(sizes) // sizes[d]
        sizes[d] = WORK_UNIT // (rest * esz) + rng.randint(1, 3)
    expand = []
    for d in range(ndim):
        if sizes[d] == 1 and rng.random() < 0.3:
            expand.append((d, rng.randint(2, 4)))
    steps = [rng.randint(1, 3) if rng.random() < 0.5 else 1 for _ in range(ndim)]
    starts = [rng.randint(0, 2) if rng.random() < 0.5 else 0 for _ in range(ndim)]
    tails = [rng.randint(0, 2) if rng.random() < 0.5 else 0 for _ in range(ndim)]

    def base_shape():
        return tuple(
            st + (n - 1) * sp + 1 + tl
            for n, sp, st, tl in zip(sizes, steps, starts, tails)
        )

    # keep the storage small: give up steps, largest dim first
    order = sorted(range(ndim), key=lambda d: -sizes[d])
    for d in order:
        if math.prod(base_shape()) * esz <= _MAX_STORAGE:
            break
        steps[d], starts[d], tails[d] = 1, 0, 0
    assert math.prod(base_shape()) * esz <= _MAX_STORAGE
    slices = tuple(
        (st, st + (n - 1) * sp + 1, sp) for n, sp, st in zip(sizes, steps, starts)
    )
    perm = None
    if ndim > 1 and rng.random() < 0.5:
        p = list(range(ndim))
        rng.shuffle(p)
        perm = tuple(p)
    r = Recipe(
        name=f"rand{k:03d}",
        dtype=dtype,
        shape=base_shape(),
        offset=rng.randint(0, 7),
        slices=slices,
        expand=tuple(expand),
        perm=perm,
    )
    view = cut(r, torch.empty(storage_numel(r), dtype=dtype))
    # an expand can push a stretched member over the cap: drop it then
    if view.numel() * esz > MAX_PAYLOAD:
        r = Recipe(r.name, dtype, r.shape, r.offset, slices, (), perm)
        view = cut(r, torch.empty(storage_numel(r), dtype=dtype))
    return Recipe(
        r.name, dtype, r.shape, r.offset, r.slices, r.expand, r.perm, "",
        expected_declines(r, view),
    )


def _random_table() -> List[Recipe]:
    rng = random.Random(_SEED)
    return [_random_recipe(rng, k) for k in range(_N_RANDOM)]


RANDOM: List[Recipe] = _random_table()
ALL: List[Recipe] = FIXED + RANDOM


def batches(recipes: List[Recipe], size: int = 32) -> List[List[Recipe]]:
    return [recipes[i : i + size] for i in range(0, len(recipes), size)]
