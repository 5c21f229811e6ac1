"""Per-tensor exponent histograms recorded at save time.

``take(..., histogram=True)`` reads every float tensor leaf once, where it
lies, and writes the distribution of ``floor(log2|x|)`` of its elements into
a small JSON sidecar beside the manifest: how many elements sit in each
binade, how many are zero, negative or non-finite. That answers what the six
moments of ``tensor_stats`` cannot: whether narrowing a leaf to float16,
bfloat16 or an fp8 format overflows, flushes or lands in the subnormal range,
for every target at once, and whether part of a gradient's mass has slid
binades down while its rms still looks healthy. Device tensors of one device
are read by ONE launch of the histogram kernel (ops/hip/staging.hip), host
tensors by torch on the CPU, in the frame of the other readers
(state_checks.py).

The histogram is of the LIVE values: a ``save_dtype`` narrowing does not
enter. The bins are float32's binades, -149..127, subnormal ones included; a
float64 element outside counts in the nearest end bin. float64, float32,
float16 and bfloat16 leaves are covered; fp8, complex, integer and quantized
leaves get no entry.
"""

from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import Any, Dict, List, Tuple

import torch

from . import state_checks
from .nonfinite import _local_tensors
from .ops.staging import (
    HIST_MAX_EXP,
    HIST_MIN_EXP,
    HIST_WORDS,
    _STATS_CLASSES,
    decode_hist,
)
from .pg_wrapper import PGWrapper
from .stateful import AppState
from .tensor_stats import _is_sharded

SIDECAR_FILENAME = ".tensor_hist"

# {logical_path: (sharded, 280 words)} for one rank
LocalReport = Dict[str, Tuple[bool, List[int]]]

_NARROW_DTYPES = (
    torch.float16,
    torch.bfloat16,
    torch.float8_e4m3fn,
    torch.float8_e5m2,
)


def _floor_log2(x: float) -> int:
    """floor(log2(x)) of a power of two or a finfo.max, exactly."""
    return math.frexp(x)[1] - 1


@dataclass(frozen=True)
class TensorHistogram:
    """The magnitudes of one leaf: ``n`` elements, of which ``n_zero`` are
    +-0 and ``n_nonfinite`` NaN or Inf; ``bins[e]`` counts the finite
    non-zero ones with ``floor(log2|x|) == e`` (non-empty bins only), and
    ``n_negative`` of those have the sign bit set."""

    n: int
    n_zero: int
    n_negative: int
    n_nonfinite: int
    bins: Dict[int, int]

    def count(self, lo: int, hi: int) -> int:
        """Finite non-zero elements with ``lo <= floor(log2|x|) < hi``."""
        return sum(c for e, c in self.bins.items() if lo <= e < hi)

    def narrowing(self, dtype: torch.dtype) -> Tuple[int, int, int]:
        """``(n_overflow, n_flushed, n_subnormal)``: how many finite non-zero
        elements a cast to ``dtype`` (float16, bfloat16, float8_e4m3fn or
        float8_e5m2) turns into Inf / NaN, turns into zero, or leaves below
        the smallest normal number.

        It is decided by binade, from ``torch.finfo``: with the largest
        value in binade M, the smallest subnormal 2^m and the smallest
        normal 2^s, overflow is ``e > M``, flushed ``e < m - 1`` and
        subnormal ``m - 1 <= e < s``. What rounding does inside the one
        binade under each threshold is not resolved: elements of binade M
        above the largest value that round up to overflow count as kept;
        all of binade m - 1 counts as subnormal, though 2^(m-1) itself and
        (for some formats' tie rule) values just above it round to zero;
        and elements of binade s - 1 that round up to 2^s count as
        subnormal."""
        if dtype not in _NARROW_DTYPES:
            raise ValueError(f"narrowing() knows {_NARROW_DTYPES}, got {dtype}")
        fi = torch.finfo(dtype)
        top = _floor_log2(fi.max)
        s = _floor_log2(fi.smallest_normal)
        m = _floor_log2(fi.smallest_normal * fi.eps)  # exact in float64
        return (
            self.count(top + 1, HIST_MAX_EXP + 1),
            self.count(HIST_MIN_EXP, m - 1),
            self.count(m - 1, s),
        )

    @property
    def exponent_range(self) -> Tuple[int, int]:
        """Lowest and highest occupied binade; (0, 0) without one."""
        return (min(self.bins, default=0), max(self.bins, default=0))


def hist_leaves(flattened: Dict[str, Any]) -> LocalReport:
    """The histogram words of every float64/32/16 and bfloat16 tensor leaf
    of ``flattened`` on this rank. Aliased leaves (tied weights) are read
    once and reported under every path; a leaf made of several local
    tensors (ShardedTensor shards) adds them."""
    unique = state_checks.UniqueTensors()
    members: Dict[str, List[int]] = {}
    sharded: Dict[str, bool] = {}
    for path, obj in flattened.items():
        locals_ = [
            t
            for t in _local_tensors(obj)
            if not t.is_quantized
            and t.layout == torch.strided
            and t.dtype in _STATS_CLASSES
            and t.device.type != "meta"
        ]
        # which ranks report a leaf is the statistics' rule
        kind = _is_sharded(obj) if locals_ else None
        if kind is None:
            continue
        sharded[path] = kind
        members[path] = [unique.add(t, None) for t in locals_]

    got = unique.read("host_tensor_hist", "hist")
    report: LocalReport = {}
    for path, idxs in members.items():
        words = [0] * HIST_WORDS
        for i in idxs:
            words = [a + b for a, b in zip(words, got[i])]
        report[path] = (sharded[path], words)
    return report


def merge_reports(found: List[LocalReport]) -> Dict[str, TensorHistogram]:
    """One entry per logical path from the ranks' reports, by rank: a
    sharded path adds every rank's words, any other path takes the lowest
    rank's that has it."""
    merged: Dict[str, List[int]] = {}
    for report in found:
        for path, (is_sharded, words) in sorted(report.items()):
            if path not in merged:
                merged[path] = list(words)
            elif is_sharded:
                merged[path] = [a + b for a, b in zip(merged[path], words)]
    return {
        path: TensorHistogram(**decode_hist(words))
        for path, words in sorted(merged.items())
    }


def collect(
    flattened: Dict[str, Any], pg_wrapper: PGWrapper
) -> Dict[str, TensorHistogram]:
    """take()'s histogram pass: read this rank's leaves, exchange the
    reports (one all_gather_object when there is more than one rank) and
    merge them; every rank returns the same result."""
    return merge_reports(state_checks.exchange(hist_leaves(flattened), pg_wrapper))


def encode_sidecar(hists: Dict[str, TensorHistogram]) -> bytes:
    """The ``.tensor_hist`` sidecar: JSON, non-empty bins only, keyed by the
    binade as a decimal string."""
    doc = {
        "version": 1,
        "histograms": {
            path: {
                "n": h.n,
                "n_zero": h.n_zero,
                "n_negative": h.n_negative,
                "n_nonfinite": h.n_nonfinite,
                "bins": {str(e): c for e, c in sorted(h.bins.items())},
            }
            for path, h in hists.items()
        },
    }
    return json.dumps(doc, indent=1, sort_keys=True).encode("utf-8")


def decode_sidecar(buf: bytes) -> Dict[str, TensorHistogram]:
    doc = json.loads(bytes(buf).decode("utf-8"))
    return {
        path: TensorHistogram(
            n=int(e["n"]),
            n_zero=int(e["n_zero"]),
            n_negative=int(e["n_negative"]),
            n_nonfinite=int(e["n_nonfinite"]),
            bins={int(k): int(c) for k, c in e["bins"].items()},
        )
        for path, e in doc["histograms"].items()
    }


def tensor_histograms(app_state: AppState) -> Dict[str, TensorHistogram]:
    """``{logical_path: TensorHistogram}`` for every float leaf of
    ``app_state`` on this rank, without collectives: what
    ``Snapshot.take(..., histogram=True)`` records, for the local rank
    only."""
    flattened, _ = state_checks.flatten_app_state(app_state, None)
    return merge_reports([hist_leaves(flattened)])
