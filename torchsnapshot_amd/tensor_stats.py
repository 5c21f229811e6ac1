"""Per-tensor value statistics recorded at save time.

``take(..., stats=True)`` reads every float tensor leaf once, where it lies,
and writes count, zeros, minimum, maximum, sum and sum of squares of its
finite elements into a small JSON sidecar beside the manifest. Someone
triaging a diverging run, or deciding whether ``save_dtype=torch.float16``
is safe for a leaf, then compares a few hundred numbers per checkpoint
instead of restoring gigabytes. Device tensors of one device are read by ONE
launch of the stats kernel (ops/hip/staging.hip), host tensors by torch on
the CPU, in the frame the non-finite scan and the replicated check share
(state_checks.py).

The statistics are of the LIVE values, in float64: a ``save_dtype``
narrowing does not enter. NaN and Inf are skipped (counting them is the
scan's job), so ``n_finite`` below the element count says they are there.
float64, float32, float16 and bfloat16 leaves are covered; fp8, complex,
integer and quantized leaves get no entry.
"""

from __future__ import annotations

import json
import math
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import state_checks
from .nonfinite import _local_tensors
from .ops.staging import (
    STATS_EMPTY,
    _STATS_CLASSES,
    decode_stats,
    merge_stats,
)
from .pg_wrapper import PGWrapper
from .stateful import AppState

SIDECAR_FILENAME = ".tensor_stats"

# {logical_path: (sharded, six words)} for one rank
LocalReport = Dict[str, Tuple[bool, List[int]]]


@dataclass(frozen=True)
class TensorStats:
    """Statistics of one leaf over its finite elements. ``min`` and ``max``
    are None when there is none."""

    n_finite: int
    n_zero: int
    min: Optional[float]
    max: Optional[float]
    sum: float
    sumsq: float

    @property
    def mean(self) -> Optional[float]:
        return self.sum / self.n_finite if self.n_finite else None

    @property
    def rms(self) -> Optional[float]:
        return math.sqrt(self.sumsq / self.n_finite) if self.n_finite else None

    @property
    def absmax(self) -> Optional[float]:
        return max(abs(self.min), abs(self.max)) if self.n_finite else None


def _is_sharded(obj: Any) -> Optional[bool]:
    """Whether the ranks hold disjoint pieces of this leaf (their statistics
    merge) or copies (the lowest rank's are taken); None for a rank whose
    piece is a copy of one that another rank reports."""
    if state_checks.is_sharded_tensor(obj):
        return True
    if not state_checks.is_dtensor(obj):
        return False
    from torch.distributed.tensor.placement_types import Replicate, Shard

    if not any(isinstance(p, Shard) for p in obj.placements):
        return False
    # sharded over some mesh dims and replicated over others: one replica
    # group reports, the one at coordinate 0 of every replicated dim
    coord = obj.device_mesh.get_coordinate() or []
    first = all(
        c == 0
        for c, p in zip(coord, obj.placements)
        if isinstance(p, Replicate)
    )
    return True if first else None


def stats_leaves(flattened: Dict[str, Any]) -> LocalReport:
    """The statistics words of every float64/32/16 and bfloat16 tensor leaf
    of ``flattened`` on this rank. Aliased leaves (tied weights) are read
    once and reported under every path; a leaf made of several local
    tensors (ShardedTensor shards) merges them in order."""
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
        kind = _is_sharded(obj) if locals_ else None
        if kind is None:
            continue
        sharded[path] = kind
        members[path] = [unique.add(t, None) for t in locals_]

    got = unique.read("host_tensor_stats", "stats")
    report: LocalReport = {}
    for path, idxs in members.items():
        words: List[int] = list(STATS_EMPTY)
        for i in idxs:
            words = merge_stats(words, got[i])
        report[path] = (sharded[path], words)
    return report


def merge_reports(found: List[LocalReport]) -> Dict[str, TensorStats]:
    """One entry per logical path from the ranks' reports, by rank: a
    sharded path merges every rank's words in rank order, any other path
    takes the lowest rank's that has it."""
    merged: Dict[str, List[int]] = {}
    for report in found:
        for path, (is_sharded, words) in sorted(report.items()):
            if path not in merged:
                merged[path] = list(words)
            elif is_sharded:
                merged[path] = merge_stats(merged[path], words)
    return {
        path: TensorStats(**decode_stats(words))
        for path, words in sorted(merged.items())
    }


def collect(
    flattened: Dict[str, Any], pg_wrapper: PGWrapper
) -> Dict[str, TensorStats]:
    """take()'s statistics pass: read this rank's leaves, exchange the
    reports (one all_gather_object when there is more than one rank) and
    merge them; every rank returns the same result."""
    return merge_reports(state_checks.exchange(stats_leaves(flattened), pg_wrapper))


def encode_sidecar(stats: Dict[str, TensorStats]) -> bytes:
    """The ``.tensor_stats`` sidecar: JSON, floats as ``float.hex()`` so
    that they read back bit for bit."""

    def hexed(x: Optional[float]) -> Optional[str]:
        return None if x is None else float(x).hex()

    doc = {
        "version": 1,
        "stats": {
            path: {
                "n_finite": s.n_finite,
                "n_zero": s.n_zero,
                "min": hexed(s.min),
                "max": hexed(s.max),
                "sum": hexed(s.sum),
                "sumsq": hexed(s.sumsq),
            }
            for path, s in stats.items()
        },
    }
    return json.dumps(doc, indent=1, sort_keys=True).encode("utf-8")


def decode_sidecar(buf: bytes) -> Dict[str, TensorStats]:
    def unhexed(x: Optional[str]) -> Optional[float]:
        return None if x is None else float.fromhex(x)

    doc = json.loads(bytes(buf).decode("utf-8"))
    return {
        path: TensorStats(
            n_finite=int(e["n_finite"]),
            n_zero=int(e["n_zero"]),
            min=unhexed(e["min"]),
            max=unhexed(e["max"]),
            sum=unhexed(e["sum"]),
            sumsq=unhexed(e["sumsq"]),
        )
        for path, e in doc["stats"].items()
    }


def tensor_stats(app_state: AppState) -> Dict[str, TensorStats]:
    """``{logical_path: TensorStats}`` for every float leaf of ``app_state``
    on this rank, without collectives: what ``Snapshot.take(...,
    stats=True)`` records, for the local rank only. Call it in a training
    loop to watch a leaf's range and norm without copying state off the
    device."""
    flattened, _ = state_checks.flatten_app_state(app_state, None)
    return merge_reports([stats_leaves(flattened)])


def relative_change(new: Optional[float], old: Optional[float]) -> Optional[float]:
    """|new - old| / |old|; inf from zero to non-zero, 0 for zero to zero,
    None when either side has no finite element."""
    if new is None or old is None:
        return None
    if old == 0:
        return 0.0 if new == 0 else math.inf
    return abs(new - old) / abs(old)
