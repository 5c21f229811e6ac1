"""The compare kernel and Snapshot.compare against torch in float64 on the
CPU (ops.staging.torch_tensor_diff): counters and max_abs exactly; the two
sums within 1e-10 relative. Both are sums of fewer than 10^5 non-negative
float64 terms, so any summation order is within (terms - 1) * 2^-53
relative, about 1e-11, plus one rounding per term.

The contiguous layout has exactly the stored sizes named; the 2-d layouts
have fixed row lengths and take the whole rows just under / over that size
(65537 one-byte elements, a prime, have no 2-d view)."""

import os
from types import SimpleNamespace

import pytest
import torch

from torchsnapshot_amd import Snapshot, StateDict
from torchsnapshot_amd.compare import CompareSink, attach_compare
from torchsnapshot_amd.io_preparers.sharded_tensor import plan_shard_reads
from torchsnapshot_amd.manifest import Shard, TensorEntry
from torchsnapshot_amd.ops import staging
from torchsnapshot_amd.scheduler import sync_execute_read_reqs
from torchsnapshot_amd.serialization import dtype_to_str
from torchsnapshot_amd.storage.fs import FSStoragePlugin

pytestmark = pytest.mark.gpu

WU = 64 * 1024
BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
PAIRS = {  # stored dtype, live dtype
    "f32": (F32, F32), "bf16": (BF16, BF16), "f16": (F16, F16),
    "f64": (torch.float64, torch.float64), "bf16-f32": (BF16, F32), "f16-f32": (F16, F32),
    "i32": (torch.int32, torch.int32), "u8": (torch.uint8, torch.uint8),
    "c64": (torch.complex64, torch.complex64),
}


@pytest.fixture(scope="module")
def engine():
    return staging.get_staging_engine(torch.device("cuda", 0))


def assert_fields(got, want):
    print("got ", got, "\nwant", want)
    assert got[:4] == want[:4]
    for g, w in zip(got[4:], want[4:]):
        assert g == w or abs(g - w) <= 1e-10 * abs(w)


def planted(stored_dt, live_dt, n):
    """(stored, live) on the CPU: live is stored in live_dt with a bit flipped
    in the first and last element and on both sides of the work-unit boundary;
    floats also get 0.0 / -0.0, two NaN payloads, inf / finite, a last-bit
    change and a large difference."""
    if stored_dt.is_floating_point:
        stored = torch.linspace(-2, 3, n, dtype=torch.float64).to(stored_dt)
        stored[5:8] = torch.tensor([0.0, float("nan"), float("inf")]).to(stored_dt)
    elif stored_dt.is_complex:
        stored = torch.view_as_complex(torch.linspace(-2, 3, 2 * n).reshape(n, 2))
    else:
        stored = (torch.arange(n) % 251).to(stored_dt)
    live = stored.to(live_dt, copy=True)
    bits = live.view(BITS[live.element_size()])
    edge = WU // stored.element_size()
    for i in {0, n - 1, min(edge - 1, n - 1), min(edge, n - 1)}:
        bits[i] ^= 1
    if stored_dt.is_floating_point:
        live[5], live[7] = -0.0, 1.0
        bits[6] ^= 1  # still a NaN
        bits[8] ^= 1
        live[9] += 1000.0
    return stored, live


@pytest.mark.parametrize("size", ["wu-1", "wu+1", "3wu+6"])
@pytest.mark.parametrize("layout", ["contiguous", "wide", "t"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_kernel_against_torch(engine, pair, layout, size):
    stored_dt, live_dt = PAIRS[pair]
    esz = stored_dt.itemsize
    n = {"wu-1": WU // esz - 1, "wu+1": WU // esz + 1, "3wu+6": 3 * WU // esz + max(6 // esz, 1)}[size]
    if layout == "contiguous":
        shape = (n,)
    else:  # whole rows: under the work unit for "wu-1", over the size else
        cols = 2064 // esz if layout == "wide" else 7
        shape = (n // cols if size == "wu-1" else -(-n // cols), cols)
        n = shape[0] * cols
    stored, live = planted(stored_dt, live_dt, n)
    if layout == "contiguous":
        view = live.cuda()
    elif layout == "wide":  # rows of >= 2 KiB stored, 8 elements between them
        view = torch.zeros(shape[0], cols + 8, dtype=live_dt, device="cuda")[:, :cols]
    else:  # transposed: narrow rows of one element
        view = torch.zeros(cols, shape[0], dtype=live_dt, device="cuda").t()
    if layout != "contiguous":
        view.copy_(live.reshape(shape))
    want = staging.torch_tensor_diff(stored.reshape(shape), live.reshape(shape))
    assert want[1] >= 2 and want[0] == n
    # the payload at offset 64 of a pinned block, and again on the device
    nbytes = 64 + n * esz
    block = staging.get_pinned_pool().acquire(nbytes)
    try:
        block.tensor[64:nbytes].copy_(stored.view(torch.uint8).reshape(-1))
        members = [(view, stored_dt, 64)]
        ((item,), _) = staging.build_compare_items(members, block.tensor.data_ptr())
        assert item is not None  # the kernel, not the torch expression
        (got,) = engine.compare(block, nbytes, members)
        (got_dev,) = engine.compare(block.tensor[:nbytes].cuda(), nbytes, members)
    finally:
        staging.get_pinned_pool().release(block)
    assert_fields(got, want)
    assert got_dev == got  # bit for bit: no word depends on the grid


def test_grid_independence(engine, monkeypatch):
    stored, live = planted(torch.float32, torch.float32, 5 * WU // 4 + 3)
    flat, view = stored.cuda().view(torch.uint8), live.cuda()
    found = []
    for grid in ("1", "3", None):
        if grid is None:
            monkeypatch.delenv("TSAMD_PACK_GRID")
        else:
            monkeypatch.setenv("TSAMD_PACK_GRID", grid)
        found.append(engine.compare(flat, flat.numel(), [(view, torch.float32, 0)])[0])
    assert found[0] == found[1] == found[2]
    assert_fields(found[0], staging.torch_tensor_diff(stored, live))


def tree_of(root):
    return {
        os.path.join(d, f): open(os.path.join(d, f), "rb").read()
        for d, _, files in os.walk(root)
        for f in files
    }


ENVS = [{}, {"TSAMD_DISABLE_BATCHING": "1"}, {"TSAMD_MAX_CHUNK_SIZE_BYTES": str(128 * 1024)}]


@pytest.mark.parametrize("env", ENVS, ids=["batched", "unbatched", "chunked"])
def test_end_to_end(tmp_path, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    torch.manual_seed(3)
    sd = StateDict(
        w=torch.randn(300, 257, device="cuda"),
        big=torch.randn(96, 1024, device="cuda"),  # 384 KiB: 3 chunks of 128 KiB
        h=torch.randn(1000, device="cuda").to(torch.bfloat16),
        idx=torch.arange(50, device="cuda"),
        step=7,
    )
    snap = Snapshot.take(str(tmp_path / "snap"), {"m": sd})
    if "TSAMD_MAX_CHUNK_SIZE_BYTES" in env:
        assert len(snap.get_manifest()["0/m/big"]["chunks"]) == 3
    files = tree_of(tmp_path)
    before = {k: sd[k].clone() for k in ("w", "big")}
    for k, where in (("w", [0, 4097, 77099]), ("big", [5, 40000, 98303])):
        sd[k].view(-1)[where] += torch.tensor([1.0, -2.5, 0.125], device="cuda")
    raw = {k: v.clone().view(torch.uint8) for k, v in sd.items() if k != "step"}
    found = snap.compare({"m": sd})
    assert set(found) == {"m/w", "m/big", "m/h", "m/idx"}
    assert found["m/h"].equal and found["m/idx"].equal
    assert found["m/h"].n == 1000 and found["m/idx"].max_abs is None
    for k in ("w", "big"):
        d = found[f"m/{k}"]
        want = (sd[k].double() - before[k].double()).abs().max().item()
        assert (d.n, d.n_diff, d.n_nonfinite_diff) == (sd[k].numel(), 3, 0)
        assert d.max_abs == want and not d.equal
    for k, v in raw.items():
        assert torch.equal(sd[k].view(torch.uint8), v)
    assert tree_of(tmp_path) == files


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_save_dtype(tmp_path, dt):
    torch.manual_seed(4)
    v = torch.randn(70001, device="cuda")
    v[:4] = torch.tensor([1.0, 0.5, 1e-30, 70000.0])
    snap = Snapshot.take(str(tmp_path / "snap"), {"m": StateDict(v=v)}, save_dtype=dt)
    d = snap.compare({"m": StateDict(v=v)})["m/v"]
    rounded = v.to(dt).float()
    assert d.n == v.numel()
    assert d.n_diff == int((rounded.view(torch.int32) != v.view(torch.int32)).sum())
    assert d.n_nonfinite_diff == int(torch.isinf(rounded).sum())
    finite = torch.isfinite(rounded)
    assert d.max_abs == (v.double() - rounded.double())[finite].abs().max().item()


def test_no_payload_copy_on_the_device(tmp_path):
    t = torch.randn(16 * 1024 * 1024, device="cuda")  # 64 MiB
    snap = Snapshot.take(str(tmp_path / "snap"), {"m": StateDict(w=t)})
    old = t[12345].item()
    t[12345] += 1
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    d = snap.compare({"m": StateDict(w=t)})["m/w"]
    rise = torch.cuda.max_memory_allocated() - before
    print("max_memory_allocated rise:", rise)
    assert rise < t.numel() * 4
    assert (d.n, d.n_diff, d.max_abs) == (t.numel(), 1, abs(t[12345].item() - old))


@pytest.mark.parametrize("dim", [0, 1], ids=["rows", "cols"])
def test_sharded(tmp_path, monkeypatch, dim):
    """2 stored shards against 3 local views: contiguous runs of the stored
    shard along dim 0 (kernel), sub-boxes along dim 1 (torch expression)."""
    torch.manual_seed(5)
    full = torch.randn(90, 66)
    n, shards = full.shape[dim], []
    at = lambda off: [off, 0] if dim == 0 else [0, off]
    for i, (off, ln) in enumerate([(0, n // 2), (n // 2, n - n // 2)]):
        piece = full.narrow(dim, off, ln).contiguous()
        (tmp_path / f"shard{i}").write_bytes(piece.numpy().tobytes())
        entry = TensorEntry(f"shard{i}", "buffer", dtype_to_str(full.dtype), list(piece.shape))
        shards.append(Shard(offsets=at(off), sizes=list(piece.shape), tensor=entry))
    live = full.clone()
    live[3, 5] += 1
    live[88, 64] -= 3
    out, targets = live.cuda(), []
    for off, ln in [(0, n // 3), (n // 3, n // 3), (2 * (n // 3), n - 2 * (n // 3))]:
        targets.append((out.narrow(dim, off, ln), at(off)))
    launches, inner = [], staging._csnap.compare_tensors
    counting = lambda flat, n, *a: launches.append(n) or inner(flat, n, *a)
    monkeypatch.setattr(staging._csnap, "compare_tensors", counting)
    sink = CompareSink()
    reqs = plan_shard_reads(shards, targets)
    attach_compare(reqs, sink, "p", SimpleNamespace(shards=shards))
    sync_execute_read_reqs(reqs, FSStoragePlugin(str(tmp_path)), 1 << 30, rank=0)
    assert sorted(launches) == ([2, 2] if dim == 0 else [])
    d = sink.result()["p"]
    got = [d.n, d.n_diff, d.n_nonfinite_diff, d.max_abs, d.sum_sq, d.ref_sum_sq]
    assert_fields(got, staging.torch_tensor_diff(full, live))
    assert torch.equal(out.cpu(), live)
