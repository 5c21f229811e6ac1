"""GPU tests: the non-finite scan kernel and the take() policy on device
state.

The oracle for every expected count is torch's CPU isnan/isinf of the same
values (after ``.to(stored)`` for the two stored classes) — never the code
under test."""

import copy
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from torchsnapshot_amd import (  # noqa: E402
    NonFiniteStateError,
    Snapshot,
    StateDict,
    find_nonfinite,
)
from torchsnapshot_amd.manifest import METADATA_FILENAME  # noqa: E402
from torchsnapshot_amd.ops import staging  # noqa: E402
from torchsnapshot_amd.test_utils import (  # noqa: E402
    check_state_dict_eq,
    tmp_snapshot_path,
)

from _nonfinite_common import (  # noqa: E402
    CLASS_IDS,
    CLASSES,
    EXPECTED_TOTALS,
    all_patterns,
    oracle,
)

NAN = float("nan")
INF = float("inf")
DEV = torch.device("cuda", 0)
WU_ELEMS = 64 * 1024 // 4  # float32 elements per 64 KiB work unit


def _scan(tensors, stored=None):
    engine = staging.get_staging_engine(DEV)
    assert engine._use_ext  # the counts below come from the kernel
    return engine.scan_nonfinite(tensors, stored)


def _items(t, stored=None):
    (its,), (cls,) = staging.build_scan_items([t], [stored])
    return its, cls


@functools.lru_cache(maxsize=None)
def _patterns(name):
    """(CPU patterns, oracle counts) of a class, computed once."""
    _, dtype, stored, _ = CLASSES[CLASS_IDS.index(name)]
    x = all_patterns(dtype)
    return x, oracle(x, stored)


def _narrow_rows(x_cpu, width=3, pitch=5, first=1):
    """``x_cpu`` (1-d) laid out on the device as rows of ``width`` elements
    inside a NaN-filled base of ``pitch`` columns: a column slice whose
    vector width can only be the element size. Padded with zeros."""
    n = x_cpu.numel()
    rows = (n + width - 1) // width
    padded = torch.zeros(rows * width, dtype=x_cpu.dtype)
    padded.view(torch.uint8)[: n * x_cpu.element_size()] = x_cpu.view(torch.uint8)
    nan_byte = 0x80 if "fnuz" in str(x_cpu.dtype) else 0xFF
    base = torch.full(
        (rows, pitch * x_cpu.element_size()), nan_byte, dtype=torch.uint8, device=DEV
    ).view(x_cpu.dtype)
    view = base[:, first : first + width]
    view.copy_(padded.view(rows, width).to(DEV))
    return view


# ---------------------------------------------------------------------------
# exhaustive patterns per class
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("name", CLASS_IDS)
def test_exhaustive_patterns_contiguous(name):
    _, _, stored, cls = CLASSES[CLASS_IDS.index(name)]
    x, want = _patterns(name)
    t = x.to(DEV)
    its, got_cls = _items(t, stored)
    assert got_cls == cls and len(its) == 1 and not its[0].outer_sizes
    got = _scan([t], [stored])
    print(name, "contiguous", got, "oracle", want)
    assert got == [want]
    if name in EXPECTED_TOTALS:
        assert got == [EXPECTED_TOTALS[name]]


@pytest.mark.parametrize("name", CLASS_IDS)
def test_exhaustive_patterns_narrow_rows(name):
    _, dtype, stored, cls = CLASSES[CLASS_IDS.index(name)]
    x, want = _patterns(name)
    t = _narrow_rows(x)
    its, got_cls = _items(t, stored)
    assert got_cls == cls and len(its) == 1
    assert its[0].vec == dtype.itemsize  # forced down to the element size
    assert its[0].outer_sizes and its[0].row_bytes < 2048
    got = _scan([t], [stored])
    print(name, "narrow rows", got, "oracle", want)
    assert got == [want]
    assert oracle(t, stored) == want  # the layout itself holds the inputs


# ---------------------------------------------------------------------------
# work-unit edges
# ---------------------------------------------------------------------------


def _edge_positions(n):
    pos = {0, n - 1}
    for b in range(WU_ELEMS, n, WU_ELEMS):
        pos.update((b - 1, b))
    return sorted(pos)


def _edge_layouts():
    contig = torch.zeros(3 * WU_ELEMS + 1, device=DEV)
    # 2064 B rows: wide, and no work-unit boundary falls on a row start
    wide = torch.zeros(97, 524, device=DEV)[:, 4:520]
    narrow = torch.zeros(16385, 8, device=DEV)[:, 1:4]  # 12 B rows
    return {"contig": contig, "wide": wide, "narrow": narrow}


@pytest.mark.parametrize("layout", ["contig", "wide", "narrow"])
def test_work_unit_edges(layout):
    t = _edge_layouts()[layout]
    its, _ = _items(t)
    it = its[0]
    if layout == "contig":
        assert it.nbytes == 3 * 65536 + 4 and not it.outer_sizes
    elif layout == "wide":
        assert it.row_bytes == 2064 and it.outer_sizes == [97]
        assert it.vec == 16
    else:
        assert it.row_bytes == 12 and it.vec == 4
    assert it.nbytes > 3 * 65536
    flat_index = torch.arange(t.numel(), device=DEV).reshape(t.shape)
    assert _scan([t]) == [(0, 0)]
    positions = _edge_positions(t.numel())
    assert len(positions) == 8 - (layout == "contig")
    for p in positions:
        # one value per run; the sliced layouts' logical order is the
        # descriptor's, so p is the flat element index the kernel sees
        t[flat_index == p] = NAN
        got = _scan([t])
        t[flat_index == p] = 0.0
        assert got == [(1, 0)], (layout, p, got)
    t[flat_index == positions[-1]] = -INF
    assert _scan([t]) == [(0, 1)]


# ---------------------------------------------------------------------------
# attribution across a batch
# ---------------------------------------------------------------------------


def _batch():
    torch.manual_seed(0)
    return [
        torch.randn(1000, device=DEV),
        torch.randn(70001, device=DEV).to(torch.bfloat16),  # > 1 work unit
        torch.randn(1, device=DEV, dtype=torch.float64),
        torch.empty(0, device=DEV, dtype=torch.float16),
        torch.randn(300, device=DEV).to(torch.float8_e5m2),
    ]


@pytest.mark.parametrize("i", range(4))
def test_batch_attribution(i):
    tensors = _batch()
    assert _scan(tensors) == [(0, 0)] * 5
    # the empty tensor takes neither value
    if tensors[i].numel():
        tensors[i][-1] = NAN
    if tensors[i + 1].numel():
        tensors[i + 1][0] = INF
    want = [oracle(t) for t in tensors]
    got = _scan(tensors)
    print(i, got, want)
    assert got == want
    assert sum(a + b for a, b in want) >= 1
    for k, w in enumerate(want):
        if k not in (i, i + 1):
            assert w == (0, 0)


# ---------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------


def _planted(*shape, dtype=torch.float32):
    torch.manual_seed(0)
    t = torch.randn(*shape).to(dtype)
    flat = t.reshape(-1)
    flat[::5] = NAN
    flat[1::7] = INF
    flat[3::11] = -INF
    return t.to(DEV)


def test_layouts():
    cases = {
        "t": _planted(130, 257).t(),
        "permute4d": _planted(6, 5, 4, 33).permute(3, 1, 0, 2),
        "expand": _planted(1, 300).expand(70, 300),
        "bf16_odd_offset": _planted(70003, dtype=torch.bfloat16)[1:],
        "strided": _planted(61, 63)[::3, ::2],
        "wide_slice": _planted(40, 1100)[:, 4:1004],
        "complex64": torch.complex(_planted(33, 9), _planted(33, 9).flip(0)).t(),
    }
    names = list(cases)
    tensors = [cases[k] for k in names]
    for k in ("t", "permute4d"):
        its, _ = _items(cases[k])
        assert not its[0].outer_sizes  # one contiguous run
    its, _ = _items(cases["expand"])
    assert its[0].outer_strides == [0]
    its, _ = _items(cases["bf16_odd_offset"])
    assert its[0].vec == 2
    want = [oracle(t) for t in tensors]
    got = _scan(tensors)
    for k, g, w in zip(names, got, want):
        print(k, g, w)
        assert w[0] > 0 and w[1] > 0
    assert got == want
    # expanded: counts multiply as torch's do
    assert want[names.index("expand")] == tuple(
        70 * c for c in oracle(_planted(1, 300))
    )


def test_declined_layout_takes_torch_path(monkeypatch):
    t = _planted(3, 3, 3, 3, 3, 3, 3, 3)[:2, :2, :2, :2, :2, :2, :2, :2]
    items, classes = staging.build_scan_items([t])
    assert items == [None] and classes == [staging.SCAN_F32]
    other = _planted(50)
    assert _scan([t, other]) == [oracle(t), oracle(other)]
    assert oracle(t)[0] > 0
    # with only declined tensors the kernel is not launched at all
    def boom(*a, **k):
        raise AssertionError("nothing to launch")

    monkeypatch.setattr(staging._csnap, "scan_nonfinite", boom)
    assert _scan([t, torch.arange(4, device=DEV)]) == [oracle(t), (0, 0)]


def test_split_under_small_cap(monkeypatch):
    monkeypatch.setattr(staging, "_KERNEL_MAX_BYTES", 4096)
    t = _planted(1000, 10)
    its, _ = _items(t)
    assert len(its) == 10 and all(it.nbytes <= 4096 for it in its)
    tt = _planted(10, 1003).t()
    assert len(_items(tt)[0]) > 1
    assert _scan([t, tt]) == [oracle(t), oracle(tt)]


def test_real_size_cap(monkeypatch):
    """A tensor of exactly 2^32 - 64 KiB bytes is one descriptor that the
    extension accepts; one row more is split. Expanded rows: the kernel
    walks 4 GiB of logical elements over 64 KiB of memory, and the counts
    are the row's times the number of rows, as torch counts an expand."""
    row = torch.zeros(1, 16384, device=DEV)
    row[0, 0] = NAN
    row[0, 16383] = INF
    row[0, 7] = -INF
    calls = []
    real = staging._csnap.scan_nonfinite

    def counting(flat, classes, n, stream, dev):
        calls.append(n)
        return real(flat, classes, n, stream, dev)

    monkeypatch.setattr(staging._csnap, "scan_nonfinite", counting)
    at_cap = row.expand(65535, 16384)
    its, _ = _items(at_cap)
    assert [it.nbytes for it in its] == [2**32 - 2**16]
    assert _scan([at_cap]) == [(65535, 2 * 65535)]
    over = row.expand(65536, 16384)
    its, _ = _items(over)
    assert len(its) > 1 and all(it.nbytes <= 2**32 - 2**16 for it in its)
    assert sum(it.nbytes for it in its) == 2**32
    assert _scan([over]) == [(65536, 2 * 65536)]
    assert calls == [1, len(its)]  # both went through the kernel


def test_disabled_extension_uses_torch(monkeypatch):
    monkeypatch.setenv("TSAMD_DISABLE_HIP_STAGING", "1")
    engine = staging.StagingEngine(DEV)
    assert not engine._use_ext

    def boom(*a, **k):
        raise AssertionError("extension disabled")

    monkeypatch.setattr(staging._csnap, "scan_nonfinite", boom)
    t = _planted(40, 30).t()
    assert engine.scan_nonfinite([t], [torch.float16]) == [oracle(t, torch.float16)]


def test_scan_is_read_only():
    tensors = [
        _planted(70000),
        _planted(50, 40)[:, 8:24],
        _planted(40, 1100, dtype=torch.float16)[:, 4:1004],
        _planted(1, 16).expand(8, 16),
    ]
    bases = [t._base if t._base is not None else t for t in tensors]
    before = [b.clone().view(torch.uint8) for b in bases]
    _scan(tensors, [torch.bfloat16, None, None, torch.float16])
    torch.cuda.synchronize()
    for b, snap in zip(bases, before):
        assert torch.equal(b.view(torch.uint8), snap)


def test_extension_refuses_bad_descriptors():
    t = torch.zeros(64, device=DEV)
    its, cls = _items(t)
    flat = staging._items_to_flat(its)
    stream = torch.cuda.current_stream().cuda_stream
    scan = staging._csnap.scan_nonfinite
    assert scan(flat, [cls], 1, stream, 0) == [0, 0]
    with pytest.raises(RuntimeError, match="unknown element class"):
        scan(flat, [9], 1, stream, 0)
    with pytest.raises(RuntimeError, match="one class code"):
        scan(flat, [], 1, stream, 0)
    bad = list(flat)
    bad[4] = 2  # vec below the float32 element size
    with pytest.raises(RuntimeError, match="below the element size"):
        scan(bad, [cls], 1, stream, 0)
    bad = list(flat)
    bad[0] += 4  # base no longer aligned to vec 16
    with pytest.raises(RuntimeError, match="not aligned"):
        scan(bad, [cls], 1, stream, 0)
    bad = list(flat)
    bad[2] = 2**32 - 2**16 + 16
    bad[3] = bad[2]
    with pytest.raises(RuntimeError, match="too large"):
        scan(bad, [cls], 1, stream, 0)
    bad = list(flat)
    bad[18] = 1  # a cast code has no business here
    with pytest.raises(RuntimeError, match="cast"):
        scan(bad, [cls], 1, stream, 0)


# ---------------------------------------------------------------------------
# save_dtype
# ---------------------------------------------------------------------------


def test_save_dtype_counts_what_is_stored():
    t = torch.tensor([1.0, 65519.99, 65520.0, -3.0], device=DEV)
    assert _scan([t]) == [(0, 0)]
    assert _scan([t], [torch.float16]) == [(0, 1)] == [oracle(t, torch.float16)]
    assert _scan([t], [torch.bfloat16]) == [(0, 0)]
    sd = StateDict(t=t)
    assert find_nonfinite({"s": sd}) == {}
    assert find_nonfinite({"s": sd}, save_dtype=torch.float16) == {"s/t": (0, 1)}
    with tmp_snapshot_path() as path:
        with pytest.raises(NonFiniteStateError) as ei:
            Snapshot.take(
                path, {"s": sd}, save_dtype=torch.float16, nonfinite="error"
            )
        assert ei.value.report == {"s/t": (0, 1, 0)}
        assert not os.path.exists(os.path.join(path, METADATA_FILENAME))
        snap = Snapshot.take(path, {"s": sd}, nonfinite="error")
        out = StateDict(t=torch.zeros(4, device=DEV))
        snap.restore({"s": out})
        assert torch.equal(out["t"], t)


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------


def _tree_bytes(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            p = os.path.join(dirpath, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


def _model_and_optim(seed):
    torch.manual_seed(seed)
    model = torch.nn.Sequential(
        torch.nn.Linear(64, 48), torch.nn.ReLU(), torch.nn.Linear(48, 8)
    ).to(DEV)
    optim = torch.optim.Adam(model.parameters(), lr=1e-3)
    model(torch.randn(16, 64, device=DEV)).sum().backward()
    optim.step()
    return model, optim


def test_take_refuses_diverged_optimizer(toggle_batching, toggle_chunking):
    model, optim = _model_and_optim(0)
    app_state = {"model": model, "optim": optim}
    with tmp_snapshot_path() as path:
        Snapshot.take(path, app_state, nonfinite="error")
        good = copy.deepcopy(
            {"model": model.state_dict(), "optim": optim.state_dict()}
        )
        before = _tree_bytes(path)
        assert METADATA_FILENAME in before
        moment = optim.state_dict()["state"][2]["exp_avg_sq"]
        moment.view(-1)[-1] = NAN
        for take in (Snapshot.take, Snapshot.async_take):
            with pytest.raises(NonFiniteStateError) as ei:
                take(path, app_state, nonfinite="error")
            assert ei.value.report == {"optim/state/2/exp_avg_sq": (1, 0, 0)}
            assert _tree_bytes(path) == before
        assert find_nonfinite(app_state) == {"optim/state/2/exp_avg_sq": (1, 0)}
        model2, optim2 = _model_and_optim(1)
        Snapshot(path).restore({"model": model2, "optim": optim2})
        assert check_state_dict_eq(model2.state_dict(), good["model"])
        assert check_state_dict_eq(optim2.state_dict(), good["optim"])


def test_dtensor_single_rank():
    import torch.distributed as dist

    created = False
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29537")
        dist.init_process_group(
            "nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0)
        )
        created = True
    try:
        from torch.distributed.device_mesh import init_device_mesh
        from torch.distributed.tensor import distribute_tensor
        from torch.distributed.tensor.placement_types import Shard

        mesh = init_device_mesh("cuda", (1,))
        full = torch.rand(512, 64, device="cuda")
        sd = StateDict(dt=distribute_tensor(full, mesh, [Shard(0)]))
        with tmp_snapshot_path() as path:
            Snapshot.take(path, {"s": sd}, nonfinite="error")
            before = _tree_bytes(path)
            bad = full.clone()
            bad[500, 63] = INF
            bad[0, 0] = NAN
            sd_bad = StateDict(dt=distribute_tensor(bad, mesh, [Shard(0)]))
            assert find_nonfinite({"s": sd_bad}) == {"s/dt": (1, 1)}
            with pytest.raises(NonFiniteStateError) as ei:
                Snapshot.take(path, {"s": sd_bad}, nonfinite="error")
            assert ei.value.report == {"s/dt": (1, 1, 0)}
            assert _tree_bytes(path) == before
            out = StateDict(
                dt=distribute_tensor(torch.zeros(512, 64, device="cuda"), mesh, [Shard(0)])
            )
            Snapshot(path).restore({"s": out})
            assert torch.equal(out["dt"].to_local(), full)
    finally:
        if created:
            dist.destroy_process_group()
