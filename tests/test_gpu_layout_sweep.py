"""GPU half of the layout sweep: every recipe of tests/_layout_sweep.py
through the five staging-kernel families, bit for bit against torch on the
CPU copy of the same storage (never the code under test).

Each launch takes a batch of at most 32 recipes. No recipe is skipped: what
a kernel path must decline is marked in the table, and the tests assert
both that it took the torch path and that its result is still right."""

import random
from dataclasses import dataclass
from typing import List

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

import _layout_sweep as L  # noqa: E402
from _layout_sweep import ALL, FIXED, Recipe  # noqa: E402

from torchsnapshot_amd import Snapshot, StateDict, _csnap, integrity  # noqa: E402
from torchsnapshot_amd.ops import staging  # noqa: E402
from torchsnapshot_amd.test_utils import (  # noqa: E402
    check_state_dict_eq,
    tmp_snapshot_path,
)

_DEV = torch.device("cuda", 0)
_STORED = [torch.bfloat16, torch.float16]
_STORED_IDS = ["bf16", "f16"]
_WORD_BASE = 12345


@dataclass
class Member:
    recipe: Recipe
    cpu_storage: torch.Tensor
    cpu_view: torch.Tensor
    storage: torch.Tensor  # on the device
    view: torch.Tensor
    want: bytes  # contiguous() bytes of the resolved CPU view


def _members(recipes, fill) -> List[Member]:
    out = []
    for r in recipes:
        cpu_storage, cpu_view = L.make(r, fill=fill)
        storage = cpu_storage.to(_DEV)
        out.append(
            Member(r, cpu_storage, cpu_view, storage, L.cut(r, storage),
                   L.ref_bytes(cpu_view))
        )
    return out


@pytest.fixture(scope="module")
def sweep() -> List[Member]:
    """Every recipe on both devices, ramp-filled; built once, never written."""
    return _members(ALL, L.ramp_fill)


@pytest.fixture(scope="module")
def f32_sweep() -> List[Member]:
    """The float32 recipes filled with values for the cast kernels."""
    return _members([r for r in ALL if r.dtype == torch.float32], L.cast_fill)


def _engine() -> staging.StagingEngine:
    assert staging.HIP_EXT_AVAILABLE
    return staging.get_staging_engine(_DEV)


def _assert_same_descriptors(cpu_items, dev_items, cpu_ms_ptrs, dev_ms_ptrs):
    """Field for field, except src_ptr, which must sit at the same offset
    from its storage."""
    assert len(cpu_items) == len(dev_items)
    for a, b, pa, pb in zip(cpu_items, dev_items, cpu_ms_ptrs, dev_ms_ptrs):
        fields = lambda it: (  # noqa: E731
            it.flat_offset, it.nbytes, it.row_bytes, it.outer_sizes,
            it.outer_strides, it.vec, it.cast,
        )
        assert fields(a) == fields(b)
        if a.nbytes:
            assert a.src_ptr - pa == b.src_ptr - pb


def _ptrs(ms, dev):
    return [(m.storage if dev else m.cpu_storage).data_ptr() for m in ms]


def _psum(payload: bytes, file_off: int) -> str:
    """CPU psum64 of ``payload`` sitting at byte ``file_off`` of a file."""
    lead = file_off % 8
    return integrity.psum64_hexdigest(
        b"\0" * lead + payload, word_base=file_off // 8
    )


def _assert_storages_unchanged(ms):
    for m in ms:
        assert L.raw_bytes(m.storage) == L.raw_bytes(m.cpu_storage), m.recipe.name


def _gather_batches(ms: List[Member]) -> List[List[Member]]:
    by_name = {m.recipe.name: m for m in ms}
    # empty members first, in the middle and last
    edge = [
        by_name[n]
        for n in ("empty", "narrow-v2", "wide-v1", "empty-3d", "contig-v1", "empty")
    ]
    return L.batches(ms) + [edge]


# ---------------------------------------------------------------------------
# a. gather
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("hash_on", [False, True], ids=["nohash", "hash"])
@pytest.mark.parametrize("mode", ["direct", "slab"])
def test_gather(mode, hash_on, sweep, monkeypatch):
    monkeypatch.setenv("TSAMD_STAGE_MODE", mode)
    engine = _engine()
    hashed = set()
    for ms in _gather_batches(sweep):
        cpu_items = staging.build_pack_items([m.cpu_view for m in ms])[0]
        dev_items = staging.build_pack_items([m.view for m in ms])[0]
        _assert_same_descriptors(
            cpu_items, dev_items, _ptrs(ms, False), _ptrs(ms, True)
        )
        batch = engine.stage([m.view for m in ms], compute_checksums=hash_on)
        try:
            # what the kernel must not be handed was resolved or materialised
            assert batch._sources is not None
            assert len(batch._sources) == len(ms)
            for m, src in zip(ms, batch._sources):
                assert not (src.is_conj() or src.is_neg()), m.recipe.name
                if "dims" in m.recipe.declines:
                    assert src.is_contiguous(), m.recipe.name
                if not m.recipe.declines or m.recipe.declines == ("stride0",):
                    assert src is m.view, m.recipe.name
            batch.wait()
            for i, m in enumerate(ms):
                assert batch.nbytes_list[i] == len(m.want), m.recipe.name
                got = bytes(batch.memoryview_of(i))
                assert got == m.want, (m.recipe.name, mode, hash_on)
            if hash_on:
                assert batch.checksums is not None
                for i, m in enumerate(ms):
                    off = batch.offsets[i]
                    assert off % 256 == 0
                    want = integrity.psum64_hexdigest(m.want, word_base=off // 8)
                    assert integrity.format_psum64(batch.checksums[i]) == want, (
                        m.recipe.name, dev_items[i].vec,
                    )
                    if m.want and not m.recipe.declines:
                        hashed.add(
                            (L.traversal_of(dev_items[i]), dev_items[i].vec)
                        )
        finally:
            batch.release()
    if hash_on:
        # the psum lane shift of the narrow vecs, in every traversal
        assert hashed == {
            (t, v)
            for t in ("contiguous", "wide", "narrow")
            for v in (16, 8, 4, 2, 1)
        }
    _assert_storages_unchanged(sweep)


# ---------------------------------------------------------------------------
# b. scatter, and the bytes around the view
# ---------------------------------------------------------------------------


def _int_view(t: torch.Tensor) -> torch.Tensor:
    """Same memory as integers: copies of it move bits, not float values."""
    if t.dtype.is_complex:
        t = torch.view_as_real(t)
    ints = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    return t.view(ints[t.element_size()])


def _scatter_batch(recipes, stored_dtypes, payloads, slab, hash_on, what):
    """One unpack_h2d launch of ``payloads`` (contiguous CPU tensors of the
    stored dtypes) into the recipes' views of 0xA5-filled device storages.
    Checks every WHOLE storage against the same copy made by torch on a
    0xA5-filled CPU storage, and the fused per-member hashes. Returns the
    launch's descriptors."""
    offsets = L.scatter_flat_offsets(recipes, [d.itemsize for d in stored_dtypes])
    raws = [L.raw_bytes(p) for p in payloads]
    total = max(o + len(b) for o, b in zip(offsets, raws)) + 256
    pinned = torch.zeros(total, dtype=torch.uint8, pin_memory=True)
    assert pinned.data_ptr() % 256 == 0
    for o, b in zip(offsets, raws):
        pinned[o : o + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8)
    targets = _members(recipes, L.byte_fill(0xA5))
    # the reference: torch's own strided copy on the CPU
    for m, p in zip(targets, payloads):
        _int_view(m.cpu_view).copy_(
            _int_view(p.to(m.recipe.dtype).reshape(m.cpu_view.shape))
        )
    items = staging.build_scatter_items(
        [m.view for m in targets], stored_dtypes, offsets,
        flat_base=pinned.data_ptr(),
    )
    _assert_same_descriptors(
        staging.build_scatter_items(
            [m.cpu_view for m in targets], stored_dtypes, offsets,
            flat_base=pinned.data_ptr(),
        ),
        items, _ptrs(targets, False), _ptrs(targets, True),
    )
    dev_slab = (
        torch.empty(total, dtype=torch.uint8, device=_DEV) if slab else None
    )
    hash_t = (
        torch.zeros(len(items), dtype=torch.uint64, device=_DEV)
        if hash_on
        else None
    )
    torch.cuda.synchronize()
    handle = _csnap.unpack_h2d(
        staging._items_to_flat(items),
        len(items),
        dev_slab.data_ptr() if slab else 0,
        pinned.data_ptr(),
        total,
        torch.cuda.current_stream().cuda_stream,
        0,
        hash_t.data_ptr() if hash_on else 0,
        _WORD_BASE * 8 if hash_on else 0,
    )
    _csnap.wait(handle)
    for m, it in zip(targets, items):
        got, want = L.raw_bytes(m.storage), L.raw_bytes(m.cpu_storage)
        if got != want:
            diff = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
            raise AssertionError(
                f"{what} {m.recipe.name} (vec {it.vec}): {len(diff)} storage "
                f"bytes differ, first at {diff[:8]}"
            )
    if hash_on:
        hashes = [int(v) % (1 << 64) for v in hash_t.cpu().tolist()]
        for m, it, b, o, h in zip(targets, items, raws, offsets, hashes):
            assert integrity.format_psum64(h) == _psum(b, _WORD_BASE * 8 + o), (
                what, m.recipe.name, it.vec,
            )
    return items


@pytest.mark.parametrize("hash_on", [False, True], ids=["nohash", "hash"])
@pytest.mark.parametrize("slab", [False, True], ids=["direct", "slab"])
def test_scatter(slab, hash_on):
    recipes = [r for r in ALL if L.kernel_scatter_ok(r) and L.payload_bytes(r)]
    assert len(recipes) > 100
    vecs = set()
    for rs in L.batches(recipes):
        payloads = [
            L.ramp_fill(r.dtype, L.payload_bytes(r) // r.dtype.itemsize)
            for r in rs
        ]
        items = _scatter_batch(
            rs, [r.dtype for r in rs], payloads, slab, hash_on, "scatter"
        )
        vecs |= {it.vec for it in items}
    assert vecs == {16, 8, 4, 2, 1}


def test_scatter_declined_recipes_take_the_torch_path(sweep):
    for m in sweep:
        plan = staging.scatter_plan(m.view, m.view.dtype)
        if m.recipe.declines or not L.is_dense(m.view):
            assert plan is None, m.recipe.name
        else:
            assert plan == staging.CAST_NONE, m.recipe.name


# ---------------------------------------------------------------------------
# c. cast gather and widen scatter
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("stored", _STORED, ids=_STORED_IDS)
@pytest.mark.parametrize("mode", ["direct", "slab"])
def test_cast_gather(mode, stored, f32_sweep, monkeypatch):
    monkeypatch.setenv("TSAMD_STAGE_MODE", mode)
    engine = _engine()
    cells = set()
    for ms in L.batches(f32_sweep):
        out_dtypes = [stored] * len(ms)
        cpu_items = staging.build_pack_items([m.cpu_view for m in ms], out_dtypes)[0]
        dev_items = staging.build_pack_items([m.view for m in ms], out_dtypes)[0]
        _assert_same_descriptors(
            cpu_items, dev_items, _ptrs(ms, False), _ptrs(ms, True)
        )
        batch = engine.stage(
            [m.view for m in ms], compute_checksums=True, out_dtypes=out_dtypes
        )
        try:
            batch.wait()
            for i, m in enumerate(ms):
                want = L.raw_bytes(L.resolved(m.cpu_view).to(stored))
                got = bytes(batch.memoryview_of(i))
                assert got == want, (m.recipe.name, dev_items[i].vec)
                h = integrity.psum64_hexdigest(
                    want, word_base=batch.offsets[i] // 8
                )
                assert integrity.format_psum64(batch.checksums[i]) == h, (
                    m.recipe.name, dev_items[i].vec,
                )
                if want and not m.recipe.declines:
                    cells.add((L.traversal_of(dev_items[i]), dev_items[i].vec))
        finally:
            batch.release()
    assert cells >= {
        (t, v) for t in ("contiguous", "wide", "narrow") for v in (16, 8, 4, 2)
    }
    _assert_storages_unchanged(f32_sweep)


@pytest.mark.parametrize("stored", _STORED, ids=_STORED_IDS)
@pytest.mark.parametrize("slab", [False, True], ids=["direct", "slab"])
def test_widen_scatter(slab, stored):
    recipes = [
        r for r in ALL
        if r.dtype == torch.float32 and L.kernel_scatter_ok(r) and L.payload_bytes(r)
    ]
    vecs = set()
    for rs in L.batches(recipes):
        payloads = [
            L.cast_fill(torch.float32, L.payload_bytes(r) // 4).to(stored)
            for r in rs
        ]
        items = _scatter_batch(rs, [stored] * len(rs), payloads, slab, True, "widen")
        assert all(it.cast != staging.CAST_NONE for it in items)
        vecs |= {it.vec for it in items}
    assert vecs == {16, 8, 4, 2}


# ---------------------------------------------------------------------------
# d. scan
# ---------------------------------------------------------------------------

_PLANTS = [float("nan"), float("inf"), float("-inf")]


def _plant(r: Recipe, view: torch.Tensor, rng: random.Random) -> None:
    """NaN and +-inf at the first and last logical elements, either side of
    each 64 KiB boundary, and at seeded positions."""
    n = view.numel()
    if n == 0 or not (view.dtype.is_floating_point or view.dtype.is_complex):
        return
    per_unit = L.WORK_UNIT // view.element_size()
    spots = {0, n - 1}
    for b in range(per_unit, n, per_unit):
        spots |= {b - 1, b}
    spots |= {rng.randrange(n) for _ in range(4)}
    for k, flat in enumerate(sorted(spots)):
        idx = tuple(int(i) for i in np.unravel_index(flat, tuple(view.shape)))
        v = _PLANTS[k % 3]
        if view.dtype.is_complex:
            v = complex(v, _PLANTS[(k + 1) % 3]) if k % 2 else complex(1.0, v)
        view[idx] = v


@pytest.fixture(scope="module")
def planted() -> List[Member]:
    rng = random.Random(7)
    out = []
    for r in ALL:
        cpu_storage, cpu_view = L.make(r, fill=L.value_fill)
        _plant(r, cpu_view, rng)
        storage = cpu_storage.to(_DEV)
        out.append(Member(r, cpu_storage, cpu_view, storage, L.cut(r, storage), b""))
    return out


def test_scan(planted):
    engine = _engine()
    nonzero = kernel = fallback = 0
    for ms in L.batches(planted):
        views = [m.view for m in ms]
        per_tensor, classes = staging.build_scan_items(views)
        cpu_items, cpu_classes = staging.build_scan_items([m.cpu_view for m in ms])
        assert classes == cpu_classes
        got = engine.scan_nonfinite(views)
        for m, its, cits, cls, g in zip(ms, per_tensor, cpu_items, classes, got):
            name = m.recipe.name
            want = staging.torch_count_nonfinite(m.cpu_view)
            assert g == want, (name, g, want)
            assert (its is None) == (cits is None), name
            if cls is None:
                assert m.recipe.dtype == torch.uint8 and g == (0, 0), name
                continue
            declined = L.scan_outer_dims(m.view) > 6 or m.recipe.lazy == "neg"
            if declined:
                # counted by the torch expression instead, same counts
                assert its is None, name
                fallback += 1
            else:
                assert its is not None, name
                _assert_same_descriptors(
                    cits, its,
                    [m.cpu_storage.data_ptr()] * len(its),
                    [m.storage.data_ptr()] * len(its),
                )
                kernel += 1
            if m.view.numel():
                assert sum(g) > 0, name
                nonzero += 1
    assert fallback >= 3 and kernel > 80 and nonzero > 100
    _assert_storages_unchanged(planted)


# ---------------------------------------------------------------------------
# e. end to end
# ---------------------------------------------------------------------------

_E2E = [
    "conj", "conj-t", "neg", "outer7", "outer8", "outer7-gaps", "stride0-outer",
    "stride0-middle", "contig-v4", "wide-v2-big", "narrow-v8-big",
    "narrow-v1", "step3-c128", "outer6", "scalar", "empty",
]


def _e2e_state():
    recipes = [r for r in FIXED if r.name in _E2E]
    assert len(recipes) == len(_E2E)
    ms = _members(recipes, L.value_fill)
    sd = StateDict({m.recipe.name: m.view for m in ms})
    want = {m.recipe.name: L.resolved(m.cpu_view).contiguous() for m in ms}
    return ms, sd, want


def test_end_to_end(toggle_batching, monkeypatch):
    monkeypatch.setenv("TSAMD_CHECKSUM", "1")
    monkeypatch.setenv("TSAMD_VERIFY_CHECKSUM", "1")
    ms, sd, want = _e2e_state()
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": sd})
        out = StateDict(
            {k: torch.zeros_like(v, device=_DEV) for k, v in want.items()}
        )
        snap.restore({"sd": out})
    assert all(v.is_cuda and v.is_contiguous() for v in out.values())
    assert check_state_dict_eq(out.state_dict(), want)
    for k, v in want.items():
        assert L.raw_bytes(out[k]) == L.raw_bytes(v), k
    _assert_storages_unchanged(ms)


def test_end_to_end_save_dtype(monkeypatch):
    monkeypatch.setenv("TSAMD_CHECKSUM", "1")
    monkeypatch.setenv("TSAMD_VERIFY_CHECKSUM", "1")
    ms, sd, want = _e2e_state()
    want = {
        k: v.to(torch.bfloat16).to(torch.float32) if v.dtype == torch.float32 else v
        for k, v in want.items()
    }
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": sd}, save_dtype=torch.bfloat16)
        out = StateDict(
            {k: torch.zeros_like(v, device=_DEV) for k, v in want.items()}
        )
        snap.restore({"sd": out})
    assert check_state_dict_eq(out.state_dict(), want)
    _assert_storages_unchanged(ms)
