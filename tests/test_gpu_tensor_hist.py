"""The histogram kernel against math.frexp on the float64 of every element on
the CPU. All 280 words are counts; every comparison is exact."""

import math
from collections import Counter

import pytest
import torch

from torchsnapshot_amd import Snapshot, StateDict
from torchsnapshot_amd.ops import staging

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32, torch.float16, torch.bfloat16]
INT_OF = {8: torch.int64, 4: torch.int32, 2: torch.int16}


def reference(t):
    """The 280 words from math.frexp on the float64 of each element."""
    x = t.detach().cpu().to(torch.float64).reshape(-1)
    finite = torch.isfinite(x)
    counted = x[finite & (x != 0)]
    # a few distinct values stand for many elements in the large tensors
    values, counts = torch.unique(counted, return_counts=True)
    words = [0] * 280
    for v, c in zip(values.tolist(), counts.tolist()):
        k = min(max(math.frexp(v)[1] - 1 + 149, 0), 276)
        words[3 + k] += c
    words[0] = int((x == 0).sum())
    words[1] = int((counted < 0).sum())
    words[2] = int((~finite).sum())
    assert words[0] + words[2] + sum(words[3:]) == t.numel()
    return words


def ramp(n, dtype):
    """A ramp through zero with -0, +0, the smallest subnormal, the largest
    finite value, NaN, +Inf and -Inf planted at the front (rotated by n, so
    that the short tensors differ) and a negative subnormal in the last
    place. 97 distinct ramp values keep the reference quick."""
    fi = torch.finfo(dtype)
    tiny = fi.smallest_normal * fi.eps
    special = [-0.0, 0.0, tiny, fi.max, math.nan, math.inf, -math.inf]
    t = (torch.arange(n, dtype=torch.float64) % 97 - 40).div(16).to(dtype)
    for i in range(min(n, len(special))):
        t[i] = special[(i + n) % len(special)]
    if n > len(special):
        t[-1] = -tiny
    return t


def from_bits(bits, dtype):
    return torch.tensor(bits, dtype=torch.int64).to(INT_OF[dtype.itemsize]).view(dtype)


@pytest.fixture(scope="module")
def engine():
    return staging.get_staging_engine(torch.device("cuda", 0))


@pytest.mark.parametrize("where", [1, 63, 64, 65, 255, 257, "wu-1", "wu", "wu+1", "3wu+17"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_work_unit_edges(engine, dtype, where):
    wu = 65536 // dtype.itemsize
    edges = {"wu-1": wu - 1, "wu": wu, "wu+1": wu + 1, "3wu+17": 3 * wu + 17}
    t = ramp(edges.get(where, where), dtype)
    assert engine.hist([t.cuda()])[0] == reference(t)


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_bin(engine, dtype):
    if dtype.itemsize == 2:
        t = from_bits(list(range(65536)), dtype)
    elif dtype == torch.float32:
        mantissas = [0, 1, 0x7FFFFF] + [1 << k for k in range(23)]
        bits = [
            sign | (e << 23) | m
            for sign in (0, 1 << 31)
            for e in range(256)
            for m in mantissas
        ]
        t = from_bits(bits, dtype)
    else:
        # every float64 binade -1074..1023: both clamped end bins are hit
        t = torch.tensor(
            [s * math.ldexp(f, e) for e in range(-1074, 1024) for f in (1.0, 1.5) for s in (1, -1)],
            dtype=dtype,
        )
    got = engine.hist([t.cuda()])[0]
    assert got == reference(t)
    lo, hi = {torch.float16: (125, 165), torch.bfloat16: (16, 277)}.get(dtype, (0, 277))
    assert all(got[3 + k] > 0 for k in range(lo, hi))


@pytest.mark.parametrize("pattern", ["normal", "subnormal", "two binades"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_contention(engine, dtype, pattern):
    """Every lane of every wave increments the same one or two counters."""
    n = 3 * (65536 // dtype.itemsize) + 17
    fi = torch.finfo(dtype)
    if pattern == "two binades":
        t = torch.tensor([0.75, -1.25], dtype=dtype).repeat(n // 2 + 1)[:n]
    else:
        value = -0.02 if pattern == "normal" else 3 * fi.smallest_normal * fi.eps
        t = torch.full((n,), value, dtype=dtype)
    got = engine.hist([t.cuda()])[0]
    assert got == reference(t)
    assert sorted(c for c in got[3:] if c) in ([n], [n // 2, n - n // 2])


@pytest.mark.parametrize("layout", ["wide", "narrow", "0-dim", "empty"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts(engine, dtype, layout):
    cols = 2048 // dtype.itemsize
    view = {
        # a column slice with rows of 2 KiB and a gap between them
        "wide": lambda: torch.zeros(37, cols + 8, dtype=dtype, device="cuda")[:, :cols],
        # rows of 24 bytes: one lane per row
        "narrow": lambda: torch.zeros(300, 50, dtype=dtype, device="cuda")[:, : 24 // dtype.itemsize],
        "0-dim": lambda: torch.zeros((), dtype=dtype, device="cuda"),
        "empty": lambda: torch.zeros(0, 5, dtype=dtype, device="cuda"),
    }[layout]()
    view.copy_(ramp(view.numel(), dtype).reshape(view.shape))
    assert engine.hist([view])[0] == reference(view)


def test_batch_and_grid_independence(engine):
    """Large, tiny and empty tensors interleaved: with 3 workgroups over the
    work units the owner changes inside every workgroup's sequence, so the
    LDS counters are flushed and reused. Each result is the tensor's own."""
    batch = [
        ramp(3 * 16384 + 17, torch.float32).cuda(),
        ramp(1, torch.float64).cuda(),
        torch.zeros(0, dtype=torch.float16, device="cuda"),
        ramp(2 * 32768 + 5, torch.bfloat16).cuda(),
        ramp(5, torch.float16).cuda(),
        ramp(8192 + 3, torch.float64).cuda(),
    ]
    alone = [engine.hist([t])[0] for t in batch]
    assert alone == [reference(t) for t in batch]
    for max_grid in (1, 3, 0):
        assert engine.hist(batch, max_grid=max_grid) == alone
        assert engine.hist(batch[::-1], max_grid=max_grid) == alone[::-1]


def test_split_pieces_add(engine, monkeypatch):
    t = ramp(40 * 1000, torch.float32).reshape(40, 1000).cuda()
    whole = engine.hist([t])[0]
    monkeypatch.setattr(staging, "_KERNEL_MAX_BYTES", 64 * 1024)
    (items,), _ = staging.build_stats_items([t])
    assert len(items) > 1
    assert engine.hist([t])[0] == whole == reference(t)


def test_round_trip(tmp_path, monkeypatch):
    model = torch.nn.Module()
    model.emb = torch.nn.Embedding(50, 16)
    model.out = torch.nn.Linear(16, 50, bias=False)
    model.out.weight = model.emb.weight
    model.register_buffer("steps", torch.arange(4))
    model.cuda()
    host = StateDict(h=ramp(100, torch.float16))
    reads, inner = [], staging.StagingEngine.hist
    counting = lambda self, ts, *a, **k: reads.append(len(ts)) or inner(self, ts, *a, **k)
    monkeypatch.setattr(staging.StagingEngine, "hist", counting)
    path = str(tmp_path / "snap")
    snap = Snapshot.take(path, {"m": model, "s": host}, histogram=True)
    recorded = snap.get_histograms()
    assert reads == [1]  # the tied weight is read once
    leaves = {"m/emb.weight": model.emb.weight, "m/out.weight": model.emb.weight, "s/h": host["h"]}
    assert set(recorded) == set(leaves)
    for name, t in leaves.items():
        assert recorded[name].__dict__ == staging.decode_hist(reference(t))
    assert (tmp_path / "snap" / ".tensor_hist").exists()
    assert not (tmp_path / "snap" / ".tensor_stats").exists()
    # the snapshot restores
    want = model.emb.weight.detach().clone()
    with torch.no_grad():
        model.emb.weight.zero_()
    snap.restore({"m": model, "s": StateDict(h=torch.zeros(100, dtype=torch.float16))})
    assert torch.equal(model.emb.weight, want)
    # a re-save without the keyword removes the sidecar
    Snapshot.take(path, {"m": model, "s": host})
    assert not (tmp_path / "snap" / ".tensor_hist").exists()
    assert Snapshot(path).get_histograms() == {}
