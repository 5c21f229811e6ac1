"""The stats kernel against a float64 reference on the CPU: counts, minimum
and maximum exactly, the sums within the worst case of n double additions
in any order plus one rounding per square, 2 * n * 2^-53 * fsum(|terms|)."""

import math

import pytest
import torch

from torchsnapshot_amd import Snapshot, tensor_stats
from torchsnapshot_amd.ops import staging

pytestmark = pytest.mark.gpu

DTYPES = [torch.float64, torch.float32, torch.float16, torch.bfloat16]


def ramp(n, dtype, values="mixed"):
    """n values on the CPU. "neg": negatives only; "nan": all NaN; "mixed":
    a ramp through zero with -0, +0, the smallest subnormal, the largest
    finite value, NaN, +Inf and -Inf planted at the front (rotated by n, so
    that the short tensors differ) and a subnormal in the last place."""
    if values == "nan":
        return torch.full((n,), math.nan, dtype=dtype)
    if values == "neg":
        return torch.linspace(-3, -0.25, n, dtype=torch.float64).to(dtype)
    fi = torch.finfo(dtype)
    tiny = fi.smallest_normal * fi.eps
    special = [-0.0, 0.0, tiny, fi.max, math.nan, math.inf, -math.inf]
    t = torch.linspace(-2, 3, n, dtype=torch.float64).to(dtype)
    for i in range(min(n, len(special))):
        t[i] = special[(i + n) % len(special)]
    if n > len(special):
        t[-1] = -tiny
    return t


def check(words, t):
    got = staging.decode_stats(words)
    x = t.detach().cpu().to(torch.float64).reshape(-1)
    x = x[torch.isfinite(x)].tolist()
    n = len(x)
    assert got["n_finite"] == n
    assert got["n_zero"] == sum(v == 0 for v in x)
    assert got["min"] == min(x, default=None)
    assert got["max"] == max(x, default=None)
    for name, terms in (("sum", x), ("sumsq", [v * v for v in x])):
        ref = math.fsum(terms)
        bound = 2 * n * 2.0**-53 * math.fsum(abs(v) for v in terms)
        err = abs(got[name] - ref)
        print(f"{name}: n={n} err={err:.3e} bound={bound:.3e}")
        # the square of float64's largest value is inf on both sides
        assert got[name] == ref or err <= bound


@pytest.fixture(scope="module")
def engine():
    return staging.get_staging_engine(torch.device("cuda", 0))


@pytest.mark.parametrize("values", ["mixed", "neg", "nan"])
@pytest.mark.parametrize("where", [1, 63, 64, 65, 255, 257, "wu-1", "wu", "wu+1", "3wu+17"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_contiguous(engine, dtype, where, values):
    wu = 65536 // dtype.itemsize
    edges = {"wu-1": wu - 1, "wu": wu, "wu+1": wu + 1, "3wu+17": 3 * wu + 17}
    n = edges.get(where, where)
    t = ramp(n, dtype, values).cuda()
    check(engine.stats([t])[0], t)


@pytest.mark.parametrize("layout", ["wide", "t", "slice", "narrow", "0-dim", "empty"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_layouts(engine, dtype, layout):
    view = {
        # rows of 2048 elements (>= 4 KiB) with a gap of 8 between them
        "wide": lambda: torch.zeros(37, 2056, dtype=dtype, device="cuda")[:, :2048],
        "t": lambda: torch.zeros(37, 53, dtype=dtype, device="cuda").t(),
        "slice": lambda: torch.zeros(64, 50, dtype=dtype, device="cuda")[:, ::2],
        # narrow rows of several elements: a load spans two or more of them
        "narrow": lambda: torch.zeros(64, 50, dtype=dtype, device="cuda")[:, :24],
        "0-dim": lambda: torch.zeros((), dtype=dtype, device="cuda"),
        "empty": lambda: torch.zeros(0, 5, dtype=dtype, device="cuda"),
    }[layout]()
    view.copy_(ramp(view.numel(), dtype).reshape(view.shape))
    check(engine.stats([view])[0], view)


def test_batch_and_grid_independence(engine):
    """One launch over a large tensor, a 1-element one and another large
    one: with 3 workgroups over 8 work units the owner changes inside every
    workgroup's sequence. Each result is the tensor's own, bit for bit, and
    no word depends on the grid."""
    batch = [
        ramp(3 * 16384 + 17, torch.float32).cuda(),
        ramp(1, torch.float64, "neg").cuda(),
        ramp(2 * 32768 + 5, torch.bfloat16).cuda(),
    ]
    alone = [engine.stats([t])[0] for t in batch]
    for max_grid in (1, 3, 0):
        assert engine.stats(batch, max_grid=max_grid) == alone
    for words, t in zip(alone, batch):
        check(words, t)


@pytest.mark.parametrize(
    "cast, classes, message",
    [
        (1, [staging.SCAN_F32], "cast descriptors not allowed"),
        (0, [staging.SCAN_E5M2], "unknown element class"),
        (0, [], "one class code per descriptor"),
    ],
)
def test_host_side_refusals(cast, classes, message):
    t = torch.zeros(64, device="cuda")
    ((item,),), _ = staging.build_stats_items([t])
    item.cast = cast
    with pytest.raises(RuntimeError, match=message):
        staging._csnap.tensor_stats(staging._items_to_flat([item]), 1, classes, 0, 0)


def test_round_trip(tmp_path, monkeypatch):
    model = torch.nn.Module()
    model.emb = torch.nn.Embedding(50, 16)
    model.out = torch.nn.Linear(16, 50, bias=False)
    model.out.weight = model.emb.weight
    model.register_buffer("steps", torch.arange(4))
    model.cuda()
    reads, inner = [], staging.StagingEngine.stats
    counting = lambda self, ts, *a, **k: reads.append(len(ts)) or inner(self, ts, *a, **k)
    monkeypatch.setattr(staging.StagingEngine, "stats", counting)
    path = str(tmp_path / "snap")
    recorded = Snapshot.take(path, {"m": model}, stats=True).get_stats()
    assert set(recorded) == {"m/emb.weight", "m/out.weight"}
    assert reads == [1]  # the tied weight is read once
    assert recorded["m/emb.weight"] == recorded["m/out.weight"]
    assert recorded == tensor_stats({"m": model})
    assert recorded["m/emb.weight"].n_finite == 50 * 16
    assert (tmp_path / "snap" / ".tensor_stats").exists()
    # without the keyword: no sidecar, and a re-save removes the old one
    Snapshot.take(str(tmp_path / "plain"), {"m": model})
    assert not (tmp_path / "plain" / ".tensor_stats").exists()
    Snapshot.take(path, {"m": model})
    assert not (tmp_path / "snap" / ".tensor_stats").exists()
    assert Snapshot(path).get_stats() == {}
