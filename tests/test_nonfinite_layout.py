"""CPU tests of the non-finite scan: a Python mirror of the kernel's
classification table and descriptor walk against torch's own CPU
isnan/isinf, the stride-order collapse, the builder's declines, and the
take()/async_take() policy end to end with host tensors."""

import logging
import os

import pytest
import torch

import torchsnapshot_amd
from torchsnapshot_amd import (
    NonFiniteStateError,
    Snapshot,
    StateDict,
    find_nonfinite,
    knobs,
    nonfinite,
)
from torchsnapshot_amd.manifest import METADATA_FILENAME
from torchsnapshot_amd.ops import staging
from torchsnapshot_amd.pg_wrapper import PGWrapper
from torchsnapshot_amd.test_utils import run_multiprocess, tmp_snapshot_path

from _nonfinite_common import (
    CLASS_IDS,
    CLASSES,
    EXPECTED_TOTALS,
    all_patterns,
    bits_to_tensor,
    mirror_count,
    oracle,
    to_bits,
    walk_items,
)

NAN = float("nan")
INF = float("inf")


# ---------------------------------------------------------------------------
# classification mirror
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("name,dtype,stored,cls", CLASSES, ids=CLASS_IDS)
def test_classification_mirror_matches_torch(name, dtype, stored, cls):
    x = all_patterns(dtype)
    want = oracle(x, stored)
    print(name, "oracle", want)
    assert mirror_count(to_bits(x), cls) == want
    assert staging.scan_class(dtype, stored) == cls
    assert staging.torch_count_nonfinite(x, stored) == want
    if name in EXPECTED_TOTALS:
        assert want == EXPECTED_TOTALS[name]
    else:
        assert want[0] > 0 and want[1] > 0


@pytest.mark.parametrize(
    "bits,stored,want",
    [
        (0x477FEFFF, torch.float16, (0, 0)),  # just below 65520.0
        (0x477FF000, torch.float16, (0, 1)),  # 65520.0: first f16 inf
        (0x7F7F7FFF, torch.bfloat16, (0, 0)),
        (0x7F7F8000, torch.bfloat16, (0, 1)),  # first bf16 inf
        (0x7F7FFFFF, torch.float16, (0, 1)),  # float32 max
        (0x7F800000, torch.bfloat16, (0, 1)),
        (0x7F800001, torch.float16, (1, 0)),
    ],
)
def test_stored_class_thresholds(bits, stored, want):
    cls = staging.scan_class(torch.float32, stored)
    for b in (bits, bits | 0x80000000):
        x = bits_to_tensor(torch.tensor([b], dtype=torch.int64), torch.float32)
        assert oracle(x, stored) == want
        assert mirror_count(to_bits(x), cls) == want
        # as float32 itself only the true inf/nan count
        assert oracle(x) == mirror_count(to_bits(x), staging.SCAN_F32)
    assert bits_to_tensor(
        torch.tensor([0x477FF000], dtype=torch.int64), torch.float32
    ).item() == 65520.0


# ---------------------------------------------------------------------------
# stride-order collapse and the descriptor walk
# ---------------------------------------------------------------------------


def _planted(*shape, dtype=torch.float32):
    """Dense tensor with NaN and Inf sprinkled at co-prime strides."""
    torch.manual_seed(0)
    t = torch.randn(*shape).to(dtype)
    flat = t.reshape(-1)
    flat[::5] = NAN
    flat[1::7] = INF
    flat[3::11] = -INF
    return t


def test_dense_permutations_collapse_to_one_run():
    for t in (
        _planted(32, 48).t(),
        _planted(8, 9, 10).permute(2, 0, 1),
        _planted(6, 5, 4, 3).permute(3, 1, 0, 2),
        _planted(4, 1, 8, 1),
    ):
        assert staging.collapse_layout_by_stride(t) == ([t.numel()], [1])
        (its,), (cls,) = staging.build_scan_items([t])
        assert cls == staging.SCAN_F32
        assert len(its) == 1 and its[0].outer_sizes == []
        assert its[0].row_bytes == its[0].nbytes == t.numel() * 4
    # the logical-order collapse must keep these apart (left alone)
    assert len(staging.collapse_layout(_planted(32, 48).t())[0]) == 2


def test_sliced_and_expanded_keep_outer_dims():
    t = _planted(50, 40)[:, 8:24]
    assert staging.collapse_layout_by_stride(t) == ([50, 16], [40, 1])
    t = _planted(1, 16).expand(8, 16)
    assert staging.collapse_layout_by_stride(t) == ([8, 16], [0, 1])
    (its,), _ = staging.build_scan_items([t])
    assert its[0].outer_sizes == [8] and its[0].outer_strides == [0]
    assert its[0].nbytes == 8 * 16 * 4
    # a transposed slice: sorted by stride, the slice's gap stays
    t = _planted(50, 40)[:, 8:24].t()
    assert staging.collapse_layout_by_stride(t) == ([50, 16], [40, 1])
    # expanded dims merge with each other, never with dense ones
    t = _planted(4).expand(2, 3, 4)
    assert staging.collapse_layout_by_stride(t) == ([6, 4], [0, 1])


_LAYOUT_CASES = [
    ("contig", lambda: _planted(64, 32)),
    ("transpose", lambda: _planted(32, 48).t()),
    ("permute3d", lambda: _planted(8, 9, 10).permute(2, 0, 1)),
    ("narrow0", lambda: _planted(100, 7)[20:60]),
    ("narrow1", lambda: _planted(50, 40)[:, 8:24]),
    ("strided", lambda: _planted(61, 63)[::3, ::2]),
    ("expanded", lambda: _planted(1, 16).expand(8, 16)),
    ("scalar", lambda: torch.tensor(INF)),
    ("flipped-ish", lambda: _planted(6, 5, 4, 3).permute(3, 1, 0, 2)),
    ("size1dims", lambda: _planted(4, 1, 8, 1)),
    ("bf16", lambda: _planted(33, 17, dtype=torch.bfloat16).t()),
    ("f16_odd_offset", lambda: _planted(67, dtype=torch.float16)[1:]),
    ("f64_cols", lambda: _planted(9, 11, dtype=torch.float64)[:, 1:4]),
    ("e5m2", lambda: _planted(13, 19, dtype=torch.float8_e5m2)[:, 3:]),
    ("complex64", lambda: torch.complex(_planted(7, 9), _planted(7, 9).flip(0)).t()),
    ("empty", lambda: torch.empty(0, 5)),
]


@pytest.mark.parametrize(
    "name,make", _LAYOUT_CASES, ids=[c[0] for c in _LAYOUT_CASES]
)
def test_descriptor_walk_matches_oracle(name, make):
    t = make()
    (its,), (cls,) = staging.build_scan_items([t])
    assert its is not None and cls is not None
    visited, nan, inf = walk_items(t, its, cls)
    want = oracle(t)
    print(name, "visited", visited, "walk", (nan, inf), "oracle", want)
    assert visited == t.numel() * (2 if t.dtype.is_complex else 1)
    assert (nan, inf) == want
    if t.numel() > 1 and name != "empty":
        assert want[0] + want[1] > 0  # the case exercises something


def test_walk_with_stored_dtype():
    t = torch.tensor([[1.0, 65519.0, 65520.0], [-7e4, NAN, 3.3e38]]).t()
    for stored in (torch.float16, torch.bfloat16):
        (its,), (cls,) = staging.build_scan_items([t], [stored])
        assert walk_items(t, its, cls)[1:] == oracle(t, stored)
    assert oracle(t, torch.float16) == (1, 3)
    assert oracle(t, torch.bfloat16) == (1, 0)
    assert oracle(t) == (1, 0)


# ---------------------------------------------------------------------------
# what the builder declines or leaves alone
# ---------------------------------------------------------------------------


def test_builder_declines():
    # 8 dims that no ordering can merge: 7 outer dims after collapsing
    t = _planted(3, 3, 3, 3, 3, 3, 3, 3)[:2, :2, :2, :2, :2, :2, :2, :2]
    assert len(staging.collapse_layout_by_stride(t)[0]) == 8
    items, classes = staging.build_scan_items([t])
    assert items == [None] and classes == [staging.SCAN_F32]
    assert staging.torch_count_nonfinite(t) == oracle(t)
    # a storage offset that splits an element: vec below the element size
    buf = bytearray(64)
    t = torch.frombuffer(buf, dtype=torch.float32, offset=2, count=8)
    t[3] = NAN
    assert t.data_ptr() % 4 == 2
    items, classes = staging.build_scan_items([t])
    assert items == [None] and classes == [staging.SCAN_F32]
    assert staging.torch_count_nonfinite(t) == (1, 0)


def test_not_scanned():
    tensors = [
        torch.arange(10),
        torch.ones(4, dtype=torch.bool),
        torch.quantize_per_tensor(torch.rand(4), 0.1, 1, torch.qint8),
        torch.eye(3).to_sparse(),
    ]
    items, classes = staging.build_scan_items(tensors)
    assert items == [None] * 4 and classes == [None] * 4
    for t in tensors:
        assert staging.torch_count_nonfinite(t) == (0, 0)
    with pytest.raises(ValueError):
        staging.build_scan_items([torch.ones(2, dtype=torch.float64)], [torch.float16])
    with pytest.raises(ValueError):
        staging.build_scan_items([torch.ones(2)], [])


def test_split_at_small_cap(monkeypatch):
    monkeypatch.setattr(staging, "_KERNEL_MAX_BYTES", 1024)
    t = _planted(100, 10)  # 4000 bytes: rows of 40, 25 rows per piece
    (its,), (cls,) = staging.build_scan_items([t])
    assert [it.nbytes for it in its] == [1000] * 4
    assert walk_items(t, its, cls) == (1000,) + oracle(t)
    # uneven tail, transposed (dim 0 is then the strided one)
    t = _planted(10, 103).t()
    (its,), (cls,) = staging.build_scan_items([t])
    assert len(its) == 5 and all(it.nbytes <= 1024 for it in its)
    assert walk_items(t, its, cls) == (1030,) + oracle(t)
    # exactly at the cap: not split
    (its,), _ = staging.build_scan_items([torch.ones(256)])
    assert len(its) == 1
    # one dim-0 row alone over the cap: declined
    items, _ = staging.build_scan_items([_planted(4, 1000)])
    assert items == [None]
    # the chunk size bounds the pieces when it is the smaller one
    with knobs.override_max_chunk_size_bytes(400):
        (its,), _ = staging.build_scan_items([_planted(100, 10)])
    assert [it.nbytes for it in its] == [400] * 10


def test_real_size_cap():
    """The builder's cap is the extension's: 2^32 - 64 KiB bytes is the
    largest single descriptor (check_descs refuses only nbytes above
    it), and anything larger is split into pieces under it."""
    cap = 2**32 - 2**16
    assert staging._KERNEL_MAX_BYTES == cap
    row = torch.zeros(1, 16384)  # expanded: no 4 GiB allocation
    (its,), _ = staging.build_scan_items([row.expand(65535, 16384)])
    assert [it.nbytes for it in its] == [cap]
    assert its[0].outer_sizes == [65535] and its[0].outer_strides == [0]
    (its,), _ = staging.build_scan_items([row.expand(65536, 16384)])
    assert len(its) > 1 and all(0 < it.nbytes <= cap for it in its)
    assert sum(it.nbytes for it in its) == 2**32
    # a 0-d or single-row tensor cannot be over the cap without a row that
    # is: declined, never handed to the extension
    wide = torch.zeros(1).expand(2, 2**30 + 1)
    assert staging.build_scan_items([wide])[0] == [None]


def test_policy_parsing(monkeypatch):
    monkeypatch.delenv("TSAMD_NONFINITE", raising=False)
    assert knobs.get_nonfinite_policy() == "ignore"
    assert nonfinite.resolve_policy(None) == "ignore"
    for p in ("ignore", "warn", "error"):
        monkeypatch.setenv("TSAMD_NONFINITE", p)
        assert nonfinite.resolve_policy(None) == p
        assert nonfinite.resolve_policy("ignore") == "ignore"
    monkeypatch.setenv("TSAMD_NONFINITE", "raise")
    with pytest.raises(ValueError):
        nonfinite.resolve_policy(None)
    assert nonfinite.resolve_policy("warn") == "warn"
    for bad in ("Error", "", "strict", True):
        with pytest.raises(ValueError):
            nonfinite.resolve_policy(bad)
    assert issubclass(NonFiniteStateError, ValueError)
    assert torchsnapshot_amd.NonFiniteStateError is nonfinite.NonFiniteStateError


# ---------------------------------------------------------------------------
# end to end, host tensors
# ---------------------------------------------------------------------------


def _good_state():
    torch.manual_seed(1)
    w = torch.randn(300, 300)  # > 256 KiB: a payload file of its own size
    return StateDict(
        w=w,
        tied=w,
        b=torch.randn(17).to(torch.bfloat16),
        idx=torch.arange(5),
        step=3,
    )


def _bad_state():
    sd = _good_state()
    sd["w"][7, 9] = NAN  # tied sees it too
    sd["step"] = 4
    return sd


def _tree_bytes(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            p = os.path.join(dirpath, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


def _restore_equals_good(path):
    good = _good_state()
    out = StateDict(
        w=torch.zeros(300, 300),
        tied=torch.zeros(300, 300),
        b=torch.zeros(17, dtype=torch.bfloat16),
        idx=torch.zeros(5, dtype=torch.int64),
        step=0,
    )
    Snapshot(path).restore({"s": out})
    for k in ("w", "tied", "b", "idx"):
        assert torch.equal(out[k], good[k]), k
    assert out["step"] == 3


def test_error_refuses_and_keeps_previous_snapshot():
    with tmp_snapshot_path() as path:
        Snapshot.take(path, {"s": _good_state()}, nonfinite="error")
        before = _tree_bytes(path)
        assert METADATA_FILENAME in before and len(before) > 1
        with pytest.raises(NonFiniteStateError) as ei:
            Snapshot.take(path, {"s": _bad_state()}, nonfinite="error")
        assert ei.value.report == {"s/w": (1, 0, 0), "s/tied": (1, 0, 0)}
        assert "s/w" in str(ei.value) and "1 NaN" in str(ei.value)
        assert isinstance(ei.value, ValueError)
        assert _tree_bytes(path) == before
        _restore_equals_good(path)
        # async_take raises from the call itself
        with pytest.raises(NonFiniteStateError) as ei:
            Snapshot.async_take(path, {"s": _bad_state()}, nonfinite="error")
        assert ei.value.report == {"s/w": (1, 0, 0), "s/tied": (1, 0, 0)}
        assert _tree_bytes(path) == before
        _restore_equals_good(path)
        # the knob is the default of the argument
        with knobs.override_env("TSAMD_NONFINITE", "error"):
            with pytest.raises(NonFiniteStateError):
                Snapshot.take(path, {"s": _bad_state()})
            Snapshot.take(path, {"s": _bad_state()}, nonfinite="ignore")
        assert _tree_bytes(path) != before


def test_error_counts_what_save_dtype_stores():
    sd = StateDict(a=torch.tensor([1.0, 65520.0, -7e4]), h=torch.ones(3, dtype=torch.float16))
    assert find_nonfinite({"s": sd}) == {}
    assert find_nonfinite({"s": sd}, save_dtype=torch.float16) == {"s/a": (0, 2)}
    assert find_nonfinite({"s": sd}, save_dtype=torch.bfloat16) == {}
    assert find_nonfinite({"s": sd}, save_dtype={"s/h": torch.float16}) == {}
    with tmp_snapshot_path() as path:
        Snapshot.take(path, {"s": sd}, nonfinite="error")
        with pytest.raises(NonFiniteStateError) as ei:
            Snapshot.take(
                path, {"s": sd}, save_dtype=torch.float16, nonfinite="error"
            )
        assert ei.value.report == {"s/a": (0, 2, 0)}
        out = StateDict(a=torch.zeros(3), h=torch.zeros(3, dtype=torch.float16))
        Snapshot(path).restore({"s": out})
        assert torch.equal(out["a"], sd["a"])


def test_find_nonfinite_leaves():
    sd = StateDict(
        p=torch.nn.Parameter(torch.tensor([NAN, 1.0])),
        f8=torch.tensor([1.0, NAN, 2.0]).to(torch.float8_e4m3fn),
        c=torch.tensor([complex(NAN, INF), complex(1, 2)]),
        i=torch.arange(3),
        nested={"m": [torch.tensor([INF, -INF, NAN], dtype=torch.float64)]},
        text="nan",
    )
    assert find_nonfinite({"s": sd}) == {
        "s/p": (1, 0),
        "s/f8": (1, 0),
        "s/c": (1, 1),  # components
        "s/nested/m/0": (1, 2),
    }


def test_warn_saves_and_logs(caplog):
    with tmp_snapshot_path() as path:
        with caplog.at_level(logging.WARNING, logger="torchsnapshot_amd.nonfinite"):
            Snapshot.take(path, {"s": _bad_state()}, nonfinite="warn")
        msgs = [r.getMessage() for r in caplog.records]
        assert len(msgs) == 1 and "s/w" in msgs[0] and "1 NaN" in msgs[0]
        out = StateDict(
            w=torch.zeros(300, 300), tied=torch.zeros(300, 300),
            b=torch.zeros(17, dtype=torch.bfloat16),
            idx=torch.zeros(5, dtype=torch.int64), step=0,
        )
        Snapshot(path).restore({"s": out})
        assert out["step"] == 4 and torch.isnan(out["w"][7, 9])
        # a finite state logs nothing
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="torchsnapshot_amd.nonfinite"):
            Snapshot.take(path, {"s": _good_state()}, nonfinite="warn")
        assert not caplog.records


def test_ignore_runs_nothing(monkeypatch, caplog):
    monkeypatch.delenv("TSAMD_NONFINITE", raising=False)
    calls = []
    real = PGWrapper.all_gather_object

    def counting(self, obj_list, obj):
        calls.append(1)
        return real(self, obj_list, obj)

    monkeypatch.setattr(PGWrapper, "all_gather_object", counting)
    with tmp_snapshot_path() as path:
        with caplog.at_level(logging.WARNING, logger="torchsnapshot_amd.nonfinite"):
            Snapshot.take(path, {"s": _bad_state()}, nonfinite="warn")
        assert caplog.records
        with_warn = len(calls)

        def boom(*a, **k):
            raise AssertionError("the scan must not run under 'ignore'")

        monkeypatch.setattr(nonfinite, "scan_leaves", boom)
        monkeypatch.setattr(nonfinite, "enforce", boom)
        monkeypatch.setattr(staging, "torch_count_nonfinite", boom)
        caplog.clear()
        del calls[:]
        Snapshot.take(path, {"s": _bad_state()}, nonfinite="ignore")
        explicit = len(calls)
        del calls[:]
        Snapshot.take(path, {"s": _bad_state()})
        Snapshot.async_take(path, {"s": _bad_state()}).wait()
        assert not caplog.records
        # world 1: the policy adds no collective even when it runs
        assert explicit == with_warn


def test_invalid_argument_raises_before_io():
    with tmp_snapshot_path() as path:
        with pytest.raises(ValueError):
            Snapshot.take(path, {"s": _good_state()}, nonfinite="strict")
        with pytest.raises(ValueError):
            Snapshot.async_take(path, {"s": _good_state()}, nonfinite="strict")
        assert not os.path.exists(path)


# ---------------------------------------------------------------------------
# world 2 (gloo)
# ---------------------------------------------------------------------------


def _world2_worker(path):
    import torch.distributed as dist

    rank = dist.get_rank()

    def state(bad):
        mine = torch.full((40,), float(rank + 1))
        if bad and rank == 1:
            mine[11] = -INF
        return StateDict(shared=torch.arange(6.0), mine=mine)

    Snapshot.take(path, {"s": state(False)}, replicated=["s/shared"])
    dist.barrier()
    before = _tree_bytes(path)
    assert METADATA_FILENAME in before

    gathers = []
    real = PGWrapper.all_gather_object

    def counting(self, obj_list, obj):
        gathers.append(1)
        return real(self, obj_list, obj)

    PGWrapper.all_gather_object = counting
    try:
        for take in (Snapshot.take, Snapshot.async_take):
            with pytest.raises(NonFiniteStateError) as ei:
                take(
                    path, {"s": state(True)}, replicated=["s/shared"],
                    nonfinite="error",
                )
            assert ei.value.report == {"s/mine": (0, 1, 1)}, ei.value.report
            assert "rank 1" in str(ei.value)
            dist.barrier()
            assert _tree_bytes(path) == before
        # exactly one more all_gather_object than an 'ignore' save
        del gathers[:]
        Snapshot.take(path + "_a", {"s": state(False)}, nonfinite="ignore")
        base = len(gathers)
        del gathers[:]
        Snapshot.take(path + "_b", {"s": state(False)}, nonfinite="error")
        assert len(gathers) == base + 1
    finally:
        PGWrapper.all_gather_object = real

    out = StateDict(shared=torch.zeros(6), mine=torch.zeros(40))
    Snapshot(path).restore({"s": out})
    assert torch.equal(out["shared"], torch.arange(6.0))
    assert torch.equal(out["mine"], torch.full((40,), float(rank + 1)))

    # distributed leaves are judged by their local part: a ShardedTensor's
    # local shards, a DTensor's to_local()
    from torch.distributed._shard import sharded_tensor
    from torch.distributed._shard.sharding_spec import ChunkShardingSpec
    from torch.distributed.device_mesh import init_device_mesh
    from torch.distributed.tensor import distribute_tensor
    from torch.distributed.tensor.placement_types import Shard

    spec = ChunkShardingSpec(dim=0, placements=["rank:0/cpu", "rank:1/cpu"])
    st = sharded_tensor.ones(spec, (8, 4))
    full = torch.ones(6, 4)
    full[5, 1] = INF  # lands in rank 1's half
    dt = distribute_tensor(full, init_device_mesh("cpu", (2,)), [Shard(0)])
    if rank == 0:
        st.local_shards()[0].tensor[1, 2] = NAN
    found = find_nonfinite({"s": StateDict(st=st, dt=dt)})
    assert found == ({"s/st": (1, 0)} if rank == 0 else {"s/dt": (0, 1)}), found
    with pytest.raises(NonFiniteStateError) as ei:
        Snapshot.take(path + "_c", {"s": StateDict(st=st, dt=dt)}, nonfinite="error")
    assert ei.value.report == {"s/st": (1, 0, 0), "s/dt": (0, 1, 1)}
    dist.barrier()
    assert not os.path.exists(path + "_c")


def test_world2_every_rank_refuses():
    with tmp_snapshot_path() as path:
        run_multiprocess(2, _world2_worker, path)
