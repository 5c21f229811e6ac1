"""CPU half of the staging-kernel layout sweep (tests/_layout_sweep.py).

What the GPU half (test_gpu_layout_sweep.py) runs through the kernels is
pinned down here without a GPU: the fixed table reaches every traversal x
vec cell of every kernel family by itself, every recipe goes through the
Python mirror of the gather arithmetic, the scatter planner declines exactly
what the table says it must, and a CPU snapshot of the awkward recipes
(lazy conj/neg views, more than six strided dims) round-trips."""

import collections

import pytest
import torch

import _layout_sweep as L
from _layout_sweep import ALL, FIXED, RANDOM, Recipe

from torchsnapshot_amd import Snapshot, StateDict
from torchsnapshot_amd.ops import staging
from torchsnapshot_amd.test_utils import check_state_dict_eq, tmp_snapshot_path

_TRAVERSALS = ("contiguous", "wide", "narrow")
_STORED = (torch.bfloat16, torch.float16)


def _plain_item(r: Recipe) -> staging.PackItem:
    _, view = L.make(r)
    return staging.build_pack_items([L.resolved(view)])[0][0]


# ---------------------------------------------------------------------------
# the table itself
# ---------------------------------------------------------------------------


def test_table_is_well_formed():
    assert len({r.name for r in ALL}) == len(ALL)
    assert len(RANDOM) == 100
    big = 0
    for r in ALL:
        storage, view = L.make(r)
        assert storage.data_ptr() % 16 == 0
        nbytes = view.numel() * view.element_size()
        assert nbytes <= L.MAX_PAYLOAD, r.name
        big += nbytes > L.WORK_UNIT
        # bytes on both sides of the view
        assert view.storage_offset() >= L.PAD, r.name
        if view.numel():
            last = view.storage_offset() + sum(
                (s - 1) * st for s, st in zip(view.shape, view.stride())
            )
            assert last < storage.numel() - L.PAD, r.name
        # the marks agree with what torch says about the view
        assert r.declines == L.expected_declines(r, view), r.name
    assert big >= 15 + 10  # one per plain cell, and some random ones
    # the ramp: distinct neighbours in every dtype
    for dtype in L.DTYPES:
        raw = L.ramp_fill(dtype, 4096).view(torch.uint8).reshape(4096, -1)
        distinct = len({bytes(row.numpy()) for row in raw})
        # 1- and 2-byte patterns repeat, but not nearby
        assert distinct >= {1: 200, 2: 3600}.get(dtype.itemsize, 4096)
        assert (raw[1:] != raw[:-1]).any(dim=1).all()


def test_same_recipes_every_time():
    assert L._random_table() == RANDOM
    dims = {len(r.shape) for r in RANDOM}
    assert dims == set(range(1, 9))
    assert {r.dtype for r in RANDOM} == set(L.DTYPES)
    assert any(r.perm for r in RANDOM) and any(r.expand for r in RANDOM)
    assert {r.offset for r in RANDOM} == set(range(8))


# ---------------------------------------------------------------------------
# coverage, from the fixed table alone
# ---------------------------------------------------------------------------


def test_fixed_table_covers_every_plain_cell():
    cells = collections.defaultdict(list)
    for r in FIXED:
        it = _plain_item(r)
        if it.nbytes:
            cells[(L.traversal_of(it), it.vec, L.size_class(it.nbytes))].append(
                r.name
            )
    missing = [
        (t, vec, size)
        for t in _TRAVERSALS
        for vec in (16, 8, 4, 2, 1)
        for size in ("small", "big")
        if not cells[(t, vec, size)]
    ]
    assert not missing, missing


def test_big_members_cut_rows_mid_row():
    """In every rows cell the > 64 KiB member's first work-unit cut falls
    inside a row, not on a row start."""
    seen = set()
    for r in FIXED:
        it = _plain_item(r)
        if it.nbytes > L.WORK_UNIT and it.outer_sizes:
            if it.row_bytes >= it.vec * 2 and L.WORK_UNIT % it.row_bytes:
                seen.add((L.traversal_of(it), it.vec))
    # narrow rows at vec 16 and 8 are the one-element rows of complex128
    # and float64: a cut cannot fall inside those
    want = {("wide", v) for v in (16, 8, 4, 2, 1)} | {
        ("narrow", v) for v in (4, 2, 1)
    }
    assert want <= seen, want - seen


def test_fixed_table_covers_every_cast_cell():
    for stored in _STORED:
        cells = set()
        for r in FIXED:
            if r.dtype != torch.float32 or r.lazy or not L.payload_bytes(r):
                continue
            _, view = L.make(r)
            it = staging.build_pack_items([view], [stored])[0][0]
            assert it.cast == staging.cast_code(torch.float32, stored)
            cells.add((L.traversal_of(it), it.vec))
        want = {(t, v) for t in _TRAVERSALS for v in (16, 8, 4, 2)}
        assert want <= cells, want - cells


def test_fixed_table_covers_every_scatter_vec():
    recipes = [r for r in FIXED if L.kernel_scatter_ok(r) and L.payload_bytes(r)]
    offs = L.scatter_flat_offsets(recipes, [r.dtype.itemsize for r in recipes])
    views = [L.make(r)[1] for r in recipes]
    # a pinned buffer is page-aligned; any 256-aligned base gives these vecs
    items = staging.build_scatter_items(
        views, [r.dtype for r in recipes], offs, flat_base=4096
    )
    cells = {(L.traversal_of(it), it.vec) for it in items}
    assert {it.vec for it in items} == {16, 8, 4, 2, 1}
    # and the flat address is what limits some of them
    plain = [_plain_item(r) for r in recipes]
    assert any(it.vec < p.vec for it, p in zip(items, plain))
    assert {t for t, _ in cells} == set(_TRAVERSALS)
    # widen items: every stored vec
    f32 = [r for r in recipes if r.dtype == torch.float32]
    offs = L.scatter_flat_offsets(f32, [2] * len(f32))
    items = staging.build_scatter_items(
        [L.make(r)[1] for r in f32], [torch.bfloat16] * len(f32), offs,
        flat_base=4096,
    )
    assert {it.vec for it in items} == {16, 8, 4, 2}
    assert {L.traversal_of(it) for it in items} == set(_TRAVERSALS)


def test_fixed_table_covers_dims_and_element_sizes():
    outer, strided_esz = set(), set()
    for r in FIXED:
        _, view = L.make(r)
        n = L.outer_dims(view) if view.numel() else 0
        if n:
            assert n == len(_plain_item(r).outer_sizes), r.name
        outer.add(n)
        if n:
            strided_esz.add(view.element_size())
    assert set(range(0, 9)) <= outer
    assert strided_esz >= {1, 2, 4, 8, 16}
    names = {r.name for r in FIXED}
    views = {r.name: L.make(r)[1] for r in FIXED}
    # the special layouts
    assert views["stride0-outer"].stride()[0] == 0
    assert views["stride0-middle"].stride()[1] == 0
    assert views["stride0-inner"].stride()[-1] == 0
    assert views["scalar"].dim() == 0 and views["empty"].numel() == 0
    assert 1 in views["size1-dims"].shape
    # rows of one element with 8- and 16-byte elements
    for name, esz in (("step2-f64", 8), ("step3-c128", 16)):
        it = _plain_item(next(r for r in FIXED if r.name == name))
        assert it.row_bytes == esz == views[name].element_size()
    assert views["conj"].is_conj() and views["conj"].is_contiguous()
    assert views["conj-t"].is_conj() and not views["conj-t"].is_contiguous()
    assert views["neg"].is_neg() and views["neg"].dtype == torch.float32
    assert {"outer7", "outer8"} <= names
    # the scan sorts dims by stride: dense permutations collapse for it,
    # so its 7- and 8-dim cases need gaps
    assert L.scan_outer_dims(views["outer8"]) == 0
    assert L.scan_outer_dims(views["outer7-gaps"]) == 7
    assert L.scan_outer_dims(views["outer8-gaps"]) == 8
    for r in ALL:
        view = L.make(r)[1]
        if view.numel() == 0 or r.dtype == torch.uint8:
            continue
        its = staging.build_scan_items([view])[0][0]
        declined = L.scan_outer_dims(view) > 6 or r.lazy == "neg"
        assert (its is None) == declined, r.name


# ---------------------------------------------------------------------------
# the Python mirror, every recipe
# ---------------------------------------------------------------------------


def test_mirror_matches_contiguous_for_every_recipe():
    for r in ALL:
        _, view = L.make(r)
        want = L.ref_bytes(view)
        assert len(want) == view.numel() * view.element_size()
        assert L.py_pack(L.resolved(view)) == want, r.name


def test_lazy_views_share_their_base_descriptors():
    """Why they have to be resolved: the descriptor of a lazy view is the
    descriptor of its base, whose bytes differ from the view's values."""
    for r in FIXED:
        if not r.lazy:
            continue
        _, view = L.make(r, fill=L.value_fill)
        base = view.conj() if r.lazy == "conj" else torch._neg_view(view)
        assert not (base.is_conj() or base.is_neg())
        assert staging.build_pack_items([view]) == staging.build_pack_items([base])
        assert L.py_pack(base) != L.ref_bytes(view), r.name
        res = staging.resolve_lazy(view)
        assert not (res.is_conj() or res.is_neg())
        assert res.dtype == view.dtype and res.numel() == view.numel()
        assert torch.equal(res, view)
    plain = torch.arange(6.0)
    assert staging.resolve_lazy(plain) is plain


def test_mirror_notices_wrong_indexing():
    """The comparison above is sensitive to the address arithmetic: each
    of these descriptor mistakes changes the mirror's bytes for some fixed
    recipe. (Indexing mutations are shown here, not on the GPU.)"""
    def mutated(mutate):
        hits = 0
        orig = staging.build_pack_items

        def patched(tensors, out_dtypes=None):
            items, offs, total = orig(tensors, out_dtypes)
            for it in items:
                mutate(it)
            return items, offs, total

        L.build_pack_items = patched
        try:
            for r in FIXED:
                _, view = L.make(r)
                try:
                    got = L.py_pack(L.resolved(view))
                except Exception:
                    got = None
                hits += got != L.ref_bytes(view)
        finally:
            L.build_pack_items = orig
        return hits

    def swap_outer(it):
        if len(it.outer_sizes) >= 2:
            it.outer_sizes[-2:] = it.outer_sizes[-2:][::-1]

    def drop_outermost_stride(it):
        if len(it.outer_strides) >= 3:
            it.outer_strides[0] = it.outer_strides[1]

    def stride0_as_1(it):
        it.outer_strides[:] = [st or 1 for st in it.outer_strides]

    assert mutated(lambda it: None) == 0
    assert mutated(swap_outer) >= 5
    assert mutated(drop_outermost_stride) >= 5
    assert mutated(stride0_as_1) >= 3


# ---------------------------------------------------------------------------
# scatter planning
# ---------------------------------------------------------------------------


def test_scatter_plan_declines_exactly_the_marked_recipes():
    """None for stride-0, more than 6 outer dims, conj and neg: the
    table's marks. The planner also declines non-dense views, for which
    torch cannot rule out overlap (docs/design.md); the scatter kernel
    itself takes those, which is what the GPU sweep runs."""
    declined = collections.Counter()
    for r in ALL:
        _, view = L.make(r)
        same = staging._scatter_layout_plan(view, view.dtype)
        if r.declines or not L.is_dense(view):
            assert same is None, r.name
            declined.update(r.declines or ("non-dense",))
        else:
            assert same == staging.CAST_NONE, r.name
        for stored, code in (
            (torch.bfloat16, staging.CAST_BF16_TO_F32),
            (torch.float16, staging.CAST_F16_TO_F32),
        ):
            got = staging._scatter_layout_plan(view, stored)
            if stored == r.dtype:
                assert got == same, r.name
            elif r.dtype == torch.float32 and same is not None:
                assert got == code, r.name
            else:
                assert got is None, r.name
    assert set(declined) == {"stride0", "dims", "lazy", "non-dense"}
    # a dense permutation is not declined for being non-contiguous
    t = next(r for r in FIXED if r.name == "outer6")
    assert staging._scatter_layout_plan(L.make(t)[1], torch.float32) == 0


# ---------------------------------------------------------------------------
# CPU round trip
# ---------------------------------------------------------------------------

_ROUND_TRIP = [
    "conj", "conj-t", "neg", "outer8", "contig-v16", "narrow-v4", "wide-v2",
]


def test_cpu_round_trip(toggle_batching):
    recipes = [r for r in FIXED if r.name in _ROUND_TRIP]
    assert len(recipes) == len(_ROUND_TRIP)
    views = {r.name: L.make(r, fill=L.value_fill)[1] for r in recipes}
    want = {k: L.resolved(v).contiguous() for k, v in views.items()}
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": StateDict(views)})
        out = StateDict({k: torch.zeros_like(v) for k, v in want.items()})
        snap.restore({"sd": out})
    assert check_state_dict_eq(out.state_dict(), want)
    for k, v in want.items():
        assert L.raw_bytes(out[k]) == L.raw_bytes(v), k


def _whole_storage_lazy():
    """Lazy views that own their whole storage, unlike the table's recipes,
    which are cut from a padded one: nothing on the save path copies such
    a tensor for being a view, so only resolving it saves its values."""
    views = {
        "conj": torch.arange(6.0).to(torch.complex64).mul(1 + 2j).conj(),
        "conj2d": torch.arange(12.0).to(torch.complex128).mul(3 - 1j)
        .reshape(3, 4).conj(),
        "neg": torch._neg_view(torch.arange(1.0, 7.0)),
        "plain": torch.arange(5.0),
    }
    for k, v in views.items():
        assert v.is_contiguous(), k
        assert v.numel() * v.element_size() == v.untyped_storage().nbytes(), k
    assert views["conj"].is_conj() and views["conj2d"].is_conj()
    assert views["neg"].is_neg()
    return views


def test_cpu_round_trip_whole_storage_lazy(toggle_batching):
    views = _whole_storage_lazy()
    want = {k: L.resolved(v).contiguous() for k, v in views.items()}
    assert want["neg"][0] == -1.0 and want["conj"][1] == 1 - 2j
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": StateDict(views)})
        out = StateDict({k: torch.zeros_like(v) for k, v in want.items()})
        snap.restore({"sd": out})
    assert check_state_dict_eq(out.state_dict(), want)
    for k, v in want.items():
        assert L.raw_bytes(out[k]) == L.raw_bytes(v), k
    # the sources still are what they were
    for k, v in views.items():
        assert torch.equal(v, want[k]) and v.is_conj() == ("conj" in k), k


def test_cpu_round_trip_whole_storage_lazy_save_dtype(toggle_batching):
    """The narrowing branch of the host stagers: a negated float32 is
    stored as bfloat16 of its values."""
    neg = torch._neg_view(torch.arange(1.0, 300.0, 1.25))
    want = L.resolved(neg).to(torch.bfloat16).to(torch.float32)
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(
            path, {"sd": StateDict(neg=neg, other=torch.arange(4.0))},
            save_dtype=torch.bfloat16,
        )
        out = StateDict(neg=torch.zeros_like(want), other=torch.zeros(4))
        snap.restore({"sd": out})
    assert torch.equal(out["neg"], want)


def test_cpu_round_trip_async_is_a_private_copy(toggle_batching):
    """An async snapshot of a lazy tensor hands storage bytes of its own:
    the source may change as soon as async_take returns. Both a view cut
    from a larger storage and tensors that own theirs."""
    r = next(r for r in FIXED if r.name == "conj")
    views = dict(_whole_storage_lazy(), cut=L.make(r, fill=L.value_fill)[1])
    want = {k: L.resolved(v).clone() for k, v in views.items()}
    with tmp_snapshot_path() as path:
        pending = Snapshot.async_take(path, {"sd": StateDict(views)})
        for v in views.values():
            v.zero_()
        snap = pending.wait()
        out = StateDict({k: torch.zeros_like(v) for k, v in want.items()})
        snap.restore({"sd": out})
    assert check_state_dict_eq(out.state_dict(), want)


@pytest.mark.parametrize("name", ["outer7", "outer8"])
def test_items_to_flat_still_refuses_what_stage_materialises(name):
    """The serializer's refusal stays; stage() is what keeps such a layout
    from reaching it."""
    r = next(r for r in FIXED if r.name == name)
    _, view = L.make(r)
    items = staging.build_pack_items([view])[0]
    with pytest.raises(ValueError, match="too complex"):
        staging._items_to_flat(items)
    flat = staging._items_to_flat(staging.build_pack_items([view.contiguous()])[0])
    assert len(flat) == 19
