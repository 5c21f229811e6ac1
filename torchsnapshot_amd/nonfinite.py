"""Non-finite state policy: scan what a snapshot is about to stage for NaN
and Inf, and refuse (or warn) before anything under the snapshot path has
been touched.

A re-save overwrites the previous payload files in place, so a diverged
model saved to a rolling path would destroy the last good copy. The scan
runs where refusing is still free: after the state has been flattened (and
shadow-cloned, for async saves), before the old commit is removed. Device
tensors of one device are counted by ONE launch of the scan kernel
(ops/hip/staging.hip); host tensors by torch on the CPU. With ``save_dtype``
the counts are those of the stored values: a finite float32 of 65520 or
more is an Inf once stored as float16.
"""

from __future__ import annotations

import logging
from typing import Any, Callable, Dict, List, Optional, Tuple

import torch

from . import knobs
from .flatten import flatten
from .pg_wrapper import PGWrapper
from .stateful import AppState

logger = logging.getLogger(__name__)

POLICIES = ("ignore", "warn", "error")

# {logical_path: (nan, inf)} for one rank; with the rank appended once
# findings have been exchanged
LocalReport = Dict[str, Tuple[int, int]]
Report = Dict[str, Tuple[int, int, int]]


class NonFiniteStateError(ValueError):
    """The state to be saved holds NaN or Inf and the policy is "error".
    ``report`` maps each offending logical path to ``(nan, inf, rank)``:
    the counts and rank of the first (lowest) rank on which that path is
    bad; a path bad on several ranks still has one entry."""

    def __init__(self, report: Report) -> None:
        self.report = dict(report)
        super().__init__(
            "refusing to snapshot non-finite state: " + _describe(self.report)
        )


def _describe(report: Report, limit: int = 5) -> str:
    parts = [
        f"{path} (rank {rank}: {nan} NaN, {inf} Inf)"
        for path, (nan, inf, rank) in list(report.items())[:limit]
    ]
    if len(report) > limit:
        parts.append(f"and {len(report) - limit} more")
    return f"{len(report)} leaves, " + "; ".join(parts)


def resolve_policy(nonfinite: Optional[str]) -> str:
    """The policy of one take() call: the argument, or the TSAMD_NONFINITE
    knob when it is None. Anything else raises ValueError."""
    if nonfinite is None:
        return knobs.get_nonfinite_policy()
    if nonfinite not in POLICIES:
        raise ValueError(
            f"nonfinite must be one of {'|'.join(POLICIES)} or None, "
            f"got {nonfinite!r}"
        )
    return nonfinite


def _local_tensors(obj: Any) -> List[torch.Tensor]:
    """The plain local tensors behind one flattened leaf."""
    if not isinstance(obj, torch.Tensor):
        return []
    try:
        from torch.distributed.tensor import DTensor

        if isinstance(obj, DTensor):
            return [obj.to_local()]
    except ImportError:
        pass
    try:
        from torch.distributed._shard.sharded_tensor import ShardedTensor

        if isinstance(obj, ShardedTensor):
            return [s.tensor for s in obj.local_shards()]
    except ImportError:
        pass
    if type(obj) is torch.Tensor or isinstance(obj, torch.nn.Parameter):
        return [obj.detach()]
    return []


def scan_leaves(
    flattened: Dict[str, Any],
    resolve_stored: Callable[[str, Any], Optional[torch.dtype]],
) -> LocalReport:
    """Count NaN and Inf in every float tensor leaf of ``flattened`` and
    return the offending ones. ``resolve_stored(path, leaf)`` names the
    dtype a leaf will be stored as (None = its own). Aliased leaves (tied
    weights) are scanned once and reported under every path."""
    from .ops import staging

    # unique tensors to scan, and which of them each path is made of
    keys: Dict[Any, int] = {}
    tensors: List[torch.Tensor] = []
    stored: List[Optional[torch.dtype]] = []
    members: Dict[str, List[int]] = {}
    for path, obj in flattened.items():
        locals_ = _local_tensors(obj)
        if not locals_:
            continue
        stored_dtype = resolve_stored(path, obj)
        for t in locals_:
            if (
                t.is_quantized
                or t.layout != torch.strided
                or not (t.dtype.is_floating_point or t.dtype.is_complex)
                or t.device.type == "meta"
            ):
                continue
            key = (
                t.data_ptr(),
                t.dtype,
                tuple(t.shape),
                tuple(t.stride()),
                str(t.device),
                stored_dtype,
            )
            if key not in keys:
                keys[key] = len(tensors)
                tensors.append(t)
                stored.append(stored_dtype)
            members.setdefault(path, []).append(keys[key])

    counts: List[Tuple[int, int]] = [(0, 0)] * len(tensors)
    by_device: Dict[int, List[int]] = {}
    for i, t in enumerate(tensors):
        if t.device.type == "cuda":
            by_device.setdefault(t.device.index or 0, []).append(i)
        else:
            counts[i] = staging.torch_count_nonfinite(t, stored[i])
    for dev_index, idxs in by_device.items():
        engine = staging.get_staging_engine(torch.device("cuda", dev_index))
        got = engine.scan_nonfinite(
            [tensors[i] for i in idxs], [stored[i] for i in idxs]
        )
        for i, c in zip(idxs, got):
            counts[i] = c

    report: LocalReport = {}
    for path, idxs in members.items():
        nan = sum(counts[i][0] for i in idxs)
        inf = sum(counts[i][1] for i in idxs)
        if nan or inf:
            report[path] = (nan, inf)
    return report


def enforce(
    policy: str, local: LocalReport, pg_wrapper: PGWrapper
) -> None:
    """Exchange the ranks' findings (one all_gather_object when there is
    more than one rank) and apply ``policy``, identically on every rank:
    "error" raises NonFiniteStateError everywhere, "warn" logs once per
    rank."""
    rank = pg_wrapper.get_rank()
    world_size = pg_wrapper.get_world_size()
    gathered: List[Optional[LocalReport]] = [None] * world_size
    if world_size > 1:
        pg_wrapper.all_gather_object(gathered, local)
    else:
        gathered[0] = local
    report: Report = {}
    for r, found in enumerate(gathered):
        for path, (nan, inf) in sorted((found or {}).items()):
            # one entry per path: the first offending rank's (a replicated
            # leaf is bad on every rank alike)
            report.setdefault(path, (nan, inf, r))
    if not report:
        return
    if policy == "error":
        raise NonFiniteStateError(report)
    logger.warning(
        "rank %d: snapshotting non-finite state: %s", rank, _describe(report)
    )


def find_nonfinite(
    app_state: AppState, save_dtype: Any = None
) -> Dict[str, Tuple[int, int]]:
    """``{logical_path: (nan, inf)}`` for every leaf of ``app_state`` that
    holds NaN or Inf on this rank; empty when the state is finite. The scan
    ``Snapshot.take(..., nonfinite=...)`` runs, for the local rank only and
    without collectives: call it in a training loop before deciding to
    checkpoint. With ``save_dtype`` (as for take) the counts are those of
    the values as they would be stored. Complex leaves count components."""
    from .snapshot import _normalize_save_dtype, _resolve_save_dtype

    rules = _normalize_save_dtype(save_dtype)
    flattened: Dict[str, Any] = {}
    for key, stateful in app_state.items():
        _, f = flatten(stateful.state_dict(), prefix=key)
        flattened.update(f)
    return scan_leaves(
        flattened, lambda path, obj: _resolve_save_dtype(rules, path, obj)
    )
