"""Tensor statistics without a GPU: the host fallback against a float64
reference, the key encoding, the cross-rank merge rule, the sidecar and the
CLI."""

import math

import pytest
import torch

from torchsnapshot_amd import Snapshot, StateDict
from torchsnapshot_amd.__main__ import main as cli_main
from torchsnapshot_amd.ops import staging
from torchsnapshot_amd.tensor_stats import TensorStats, decode_sidecar
from torchsnapshot_amd.tensor_stats import encode_sidecar, merge_reports


def reference(t):
    """(n_finite, n_zero, min, max, sum terms, square terms) in float64."""
    x = t.detach().cpu().to(torch.float64).reshape(-1)
    x = x[torch.isfinite(x)].tolist()
    zeros = sum(v == 0 for v in x)
    return len(x), zeros, min(x, default=None), max(x, default=None), x, [v * v for v in x]


@pytest.mark.parametrize(
    "dtype", [torch.float64, torch.float32, torch.float16, torch.bfloat16]
)
def test_host_fallback_matches_reference(dtype):
    fi = torch.finfo(dtype)
    t = torch.linspace(-3, 2, 1000, dtype=torch.float64).to(dtype)
    special = [0.0, -0.0, fi.smallest_normal * fi.eps, math.nan, math.inf, -math.inf]
    t[:6] = torch.tensor(special, dtype=dtype)
    got = staging.decode_stats(staging.host_tensor_stats(t.reshape(40, 25).t()))
    n, nz, lo, hi, terms, squares = reference(t)
    assert (got["n_finite"], got["n_zero"], got["min"], got["max"]) == (n, nz, lo, hi)
    for value, ts in ((got["sum"], terms), (got["sumsq"], squares)):
        bound = 2 * n * 2.0**-53 * math.fsum(abs(v) for v in ts)
        assert abs(value - math.fsum(ts)) <= bound
    nans = torch.full((3,), math.nan, dtype=dtype)
    assert staging.decode_stats(staging.host_tensor_stats(nans))["min"] is None


def test_key_round_trip_and_order():
    tiny, big = 5e-324, 1.7976931348623157e308
    values = [-big, -1.0, -tiny, -0.0, 0.0, tiny, 1.0, big]
    keys = [staging.stats_key(v) for v in values]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    for v, k in zip(values, keys):
        back = staging.stats_unkey(k)
        assert back == v and math.copysign(1.0, back) == math.copysign(1.0, v)
        assert 0 < k < 2**64 - 1  # never one of the two "empty" words


def test_merge_rule_replicated_and_sharded():
    def words(n, nz, lo, hi, s, q):
        return [
            n, nz, staging.stats_key(lo), staging.stats_key(hi),
            staging._f64_bits(s), staging._f64_bits(q),
        ]

    rank0 = {"m/rep": (False, words(4, 1, -1.0, 2.0, 3.0, 9.0)),
             "m/shard": (True, words(2, 0, 1.0, 5.0, 6.0, 26.0))}
    rank1 = {"m/rep": (False, words(4, 0, -7.0, 7.0, 0.5, 99.0)),
             "m/shard": (True, words(3, 2, -4.0, 0.0, -4.0, 16.0)),
             "m/only1": (False, list(staging.STATS_EMPTY))}
    merged = merge_reports([rank0, rank1])
    assert merged["m/rep"] == TensorStats(4, 1, -1.0, 2.0, 3.0, 9.0)
    assert merged["m/shard"] == TensorStats(5, 2, -4.0, 5.0, 2.0, 42.0)
    assert merged["m/only1"] == TensorStats(0, 0, None, None, 0.0, 0.0)
    shard = merged["m/shard"]
    assert (shard.mean, shard.absmax, shard.rms) == (0.4, 5.0, math.sqrt(42.0 / 5))
    assert merged["m/only1"].rms is None


def test_sidecar_round_trip():
    stats = {
        "a/w": TensorStats(3, 1, -0.0, 0.1, 0.1 + 0.2, 1e-310),
        "a/none": TensorStats(0, 0, None, None, 0.0, 0.0),
    }
    back = decode_sidecar(encode_sidecar(stats))
    assert back == stats
    assert math.copysign(1.0, back["a/w"].min) == -1.0


def test_cli_and_take_on_host_tensors(tmp_path, capsys):
    w = torch.arange(-4, 4, dtype=torch.float32)
    state = {"s": StateDict(w=w, steps=torch.arange(3), lr=0.5)}
    with pytest.raises(TypeError):
        Snapshot.take(str(tmp_path / "x"), state, None, None, None, None, None, None, None, True)
    old = Snapshot.take(str(tmp_path / "old"), state, stats=True)
    assert old.get_stats() == {"s/w": TensorStats(8, 1, -4.0, 3.0, -4.0, 44.0)}
    state["s"]["w"] = w * 2
    new = Snapshot.take(str(tmp_path / "new"), state, stats=True)
    assert cli_main(["stats", new.path, "--against", old.path]) == 0
    out = capsys.readouterr().out
    assert "s/w: n_finite=8 n_zero=1 min=-8 max=6" in out
    assert "d_rms=1 d_absmax=1" in out
    # a re-save without stats removes the sidecar, and the CLI says so
    Snapshot.take(new.path, state)
    assert Snapshot(new.path).get_stats() == {}
    assert not (tmp_path / "new" / ".tensor_stats").exists()
    assert cli_main(["stats", new.path]) == 1
