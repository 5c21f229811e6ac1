"""Exponent histograms without a GPU: the host fallback against math.frexp,
the record's queries, the cross-rank merge rule, the sidecar and the CLI."""

import math

import pytest
import torch

from torchsnapshot_amd import Snapshot, StateDict, TensorHistogram
from torchsnapshot_amd.__main__ import main as cli_main
from torchsnapshot_amd.ops import staging
from torchsnapshot_amd.tensor_hist import decode_sidecar, encode_sidecar, merge_reports

DTYPES = [torch.float64, torch.float32, torch.float16, torch.bfloat16]


def reference(t):
    """The 280 words from math.frexp on the float64 of each element."""
    words = [0] * 280
    for v in t.detach().to(torch.float64).reshape(-1).tolist():
        if v == 0:
            words[0] += 1
        elif not math.isfinite(v):
            words[2] += 1
        else:
            words[1] += v < 0
            words[3 + min(max(math.frexp(v)[1] - 1 + 149, 0), 276)] += 1
    return words


@pytest.mark.parametrize("dtype", DTYPES)
def test_host_fallback_matches_reference(dtype):
    fi = torch.finfo(dtype)
    tiny = fi.smallest_normal * fi.eps
    t = torch.linspace(-3, 2, 1000, dtype=torch.float64).to(dtype)
    special = [0.0, -0.0, tiny, -tiny, fi.max, -fi.smallest_normal, math.nan, math.inf, -math.inf]
    t[: len(special)] = torch.tensor(special, dtype=dtype)
    got = staging.host_tensor_hist(t.reshape(40, 25).t())
    assert got == reference(t)
    assert got[0] + got[2] + sum(got[3:]) == t.numel()
    assert staging.decode_hist(got)["n"] == t.numel()


def test_count_and_sidecar_round_trip():
    h = TensorHistogram(n=20, n_zero=3, n_negative=4, n_nonfinite=1, bins={-149: 2, -3: 5, 0: 8, 127: 1})
    assert (h.count(-3, 1), h.count(-149, -3), h.count(1, 127), h.count(-200, 200)) == (13, 2, 0, 16)
    hists = {"a/w": h, "a/none": TensorHistogram(0, 0, 0, 0, {})}
    assert decode_sidecar(encode_sidecar(hists)) == hists


@pytest.mark.parametrize(
    "dtype", [torch.float16, torch.bfloat16, torch.float8_e4m3fn, torch.float8_e5m2]
)
def test_narrowing_matches_the_cast(dtype):
    """1.25 * 2^e rounds across no binade in any of the targets, so the
    counts by binade are the counts of the cast itself."""
    values = [s * math.ldexp(1.25, e) for e in range(-147, 128) for s in (1, -1)]
    t = torch.tensor(values + [0.0, -0.0, 0.0], dtype=torch.float64)
    cast = t.to(dtype).to(torch.float64)
    nonzero = t != 0
    want = (
        int((~torch.isfinite(cast)).sum()),
        int(((cast == 0) & nonzero).sum()),
        int(((cast != 0) & (cast.abs() < torch.finfo(dtype).smallest_normal)).sum()),
    )
    h = TensorHistogram(**staging.decode_hist(staging.host_tensor_hist(t)))
    assert h.narrowing(dtype) == want
    assert all(c > 0 for c in want[1:]) and h.n_zero == 3


def test_merge_rule_replicated_and_sharded():
    def words(zero, neg, nonfinite, **bins):
        w = [zero, neg, nonfinite] + [0] * 277
        for k, c in bins.items():
            w[3 + int(k[1:])] = c
        return w

    rank0 = {"m/rep": (False, words(1, 2, 0, k149=5)), "m/shard": (True, words(0, 1, 1, k149=2, k150=3))}
    rank1 = {
        "m/rep": (False, words(9, 9, 9, k0=9)),
        "m/shard": (True, words(2, 0, 0, k150=4, k276=1)),
        "m/only1": (False, words(0, 0, 0)),
    }
    merged = merge_reports([rank0, rank1])
    assert merged["m/rep"] == TensorHistogram(6, 1, 2, 0, {0: 5})
    assert merged["m/shard"] == TensorHistogram(13, 2, 1, 1, {0: 2, 1: 7, 127: 1})
    assert merged["m/only1"] == TensorHistogram(0, 0, 0, 0, {})


def test_cli_and_take_on_host_tensors(tmp_path, capsys):
    w = torch.tensor([-4.0, -0.0, 0.5, 3.0, 70000.0, 1e-8, math.inf])
    state = {"s": StateDict(w=w, steps=torch.arange(3), lr=0.5)}
    snap = Snapshot.take(str(tmp_path / "snap"), state, histogram=True)
    want = TensorHistogram(7, 1, 1, 1, {2: 1, -1: 1, 1: 1, 16: 1, -27: 1})
    assert snap.get_histograms() == {"s/w": want}
    assert not (tmp_path / "snap" / ".tensor_stats").exists()
    assert cli_main(["hist", snap.path, "s/*", "--narrow", "float16"]) == 0
    out = capsys.readouterr().out
    assert "s/w: n=7 exponents=2^-27..2^16 n_zero=1 n_negative=1 n_nonfinite=1" in out
    assert "float16: overflow=1 flushed=1 subnormal=0" in out
    assert cli_main(["hist", snap.path, "nothing/*"]) == 0
    assert capsys.readouterr().out == ""
    # a re-save without the keyword removes the sidecar, and the CLI says so
    Snapshot.take(snap.path, state)
    assert Snapshot(snap.path).get_histograms() == {}
    assert not (tmp_path / "snap" / ".tensor_hist").exists()
    assert cli_main(["hist", snap.path]) == 1
