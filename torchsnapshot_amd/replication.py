"""Replicated-state check: compare what the ranks are about to store for
every leaf that is claimed to be replicated, and refuse (or warn) before
anything under the snapshot path has been touched.

``replicated=`` globs and the automatic marking of DistributedDataParallel
subtrees tell take() that a leaf is bit-identical on all ranks; one rank
then writes it and the others drop their copies. If the ranks have drifted,
the snapshot would silently keep one rank's values. The check runs beside
the non-finite scan, where refusing is still free: each rank fingerprints
its copy (the psum64 of the bytes as they would be stored; device tensors
of one device by ONE launch of the fingerprint kernel in
ops/hip/staging.hip, which reads them in place), one all_gather_object
exchanges the fingerprints, and every rank takes the same decision.
"""

from __future__ import annotations

import logging
from typing import Any, Dict, Iterable, List, Optional, Tuple

import torch

from . import knobs, state_checks
from .integrity import format_psum64
from .pg_wrapper import PGWrapper
from .stateful import AppState

logger = logging.getLogger(__name__)

POLICIES = state_checks.POLICIES

# {logical_path: (fingerprint hex, stored dtype, shape)} for one rank
Finding = Tuple[str, str, Tuple[int, ...]]
LocalReport = Dict[str, Finding]
# {logical_path: [fingerprint hex of rank 0, of rank 1, ...]}
Report = Dict[str, List[str]]


class ReplicatedStateMismatchError(ValueError):
    """State marked as replicated differs between ranks and the policy is
    "error". ``report`` maps each offending logical path to the list of its
    fingerprints, one per rank."""

    def __init__(self, report: Report, detail: str) -> None:
        self.report = {p: list(v) for p, v in report.items()}
        super().__init__(
            "refusing to snapshot: state marked as replicated differs "
            "between ranks: " + detail
        )


def resolve_policy(replicated_check: Optional[str]) -> str:
    """The policy of one take() call: the argument, or the
    TSAMD_REPLICATED_CHECK knob when it is None. Anything else raises
    ValueError."""
    return state_checks.resolve_policy(
        replicated_check, "replicated_check", knobs.get_replicated_check_policy
    )


def _local_tensor(obj: Any, dtensor_local: bool) -> Optional[torch.Tensor]:
    """The tensor to fingerprint behind one flattened leaf, or None: plain
    tensors and Parameters, and a DTensor's local shard when asked for."""
    if not isinstance(obj, torch.Tensor):
        return None
    if state_checks.is_dtensor(obj):
        return obj.to_local().detach() if dtensor_local else None
    if state_checks.is_plain_tensor(obj):
        return obj.detach()
    return None  # ShardedTensor and other subclasses


def _fingerprint_leaves(
    flattened: Dict[str, Any],
    paths: Iterable[str],
    resolve_stored: state_checks.ResolveStored,
    dtensor_local: bool,
) -> LocalReport:
    # unique tensors to fingerprint, and which of them each path is
    unique = state_checks.UniqueTensors()
    member: Dict[str, int] = {}
    for path in sorted(paths):
        t = _local_tensor(flattened.get(path), dtensor_local)
        if t is None or t.device.type == "meta":
            continue
        member[path] = unique.add(t, resolve_stored(path, flattened[path]))

    sums = unique.read("host_fingerprint", "fingerprint")
    return {
        path: (
            format_psum64(sums[i]),
            str(unique.stored[i] or unique.tensors[i].dtype),
            tuple(unique.tensors[i].shape),
        )
        for path, i in member.items()
    }


def fingerprint_leaves(
    flattened: Dict[str, Any],
    paths: Iterable[str],
    resolve_stored: state_checks.ResolveStored,
) -> LocalReport:
    """``{path: (hex, stored dtype, shape)}`` for the plain tensor and
    Parameter leaves among ``paths``: the psum64 of the bytes each would be
    stored as. ``resolve_stored(path, leaf)`` names the dtype a leaf will be
    stored as (None = its own). Aliased leaves are fingerprinted once;
    device tensors take one kernel launch per device, host tensors the host
    hash. DTensor and ShardedTensor leaves are skipped (their preparers
    choose writers from placements, not from the replicated claim), and so
    is anything that is not a tensor."""
    return _fingerprint_leaves(flattened, paths, resolve_stored, False)


def _describe(gathered: List[LocalReport], bad: List[str], limit: int = 5) -> str:
    parts = []
    for path in bad[:limit]:
        found = [g.get(path) for g in gathered]
        ranks = [r for r, f in enumerate(found) if f != found[0]]
        what = "fingerprint"
        if any(f is None or found[0] is None or f[1:] != found[0][1:] for f in found):
            what = "shape or stored dtype"
        parts.append(
            f"{path} ({what} of rank{'s' if len(ranks) > 1 else ''} "
            f"{', '.join(map(str, ranks))} differs from rank 0's)"
        )
    if len(bad) > limit:
        parts.append(f"and {len(bad) - limit} more")
    return f"{len(bad)} leaves, " + "; ".join(parts)


def enforce(policy: str, local: LocalReport, pg_wrapper: PGWrapper) -> None:
    """Exchange the ranks' fingerprints (one all_gather_object) and apply
    ``policy``, identically on every rank. A path is bad when its
    (fingerprint, stored dtype, shape) is not the same on all ranks:
    "error" raises ReplicatedStateMismatchError everywhere, "warn" logs
    once per rank."""
    rank = pg_wrapper.get_rank()
    found = state_checks.exchange(local, pg_wrapper)
    bad = sorted(
        path
        for path in set().union(*found)
        if any(f.get(path) != found[0].get(path) for f in found[1:])
    )
    if not bad:
        return
    report: Report = {
        path: [f[path][0] if path in f else "missing" for f in found]
        for path in bad
    }
    detail = _describe(found, bad)
    if policy == "error":
        raise ReplicatedStateMismatchError(report, detail)
    logger.warning(
        "rank %d: state marked as replicated differs between ranks; rank "
        "0's copy is kept: %s",
        rank,
        detail,
    )


def fingerprint_state(
    app_state: AppState, save_dtype: Any = None
) -> Dict[str, str]:
    """``{logical_path: "psum64:<hex>"}`` for every plain tensor, Parameter
    and DTensor-local leaf of ``app_state`` on this rank, without
    collectives: the fingerprint ``Snapshot.take(..., replicated_check=...)``
    compares across ranks. It is the checksum of the leaf's bytes in
    logical order and does not depend on strides, so it answers "did
    anything change since the last step?" and "do two runs agree?" without
    copying state off the device. With ``save_dtype`` (as for take) it is
    the fingerprint of what would be stored."""
    flattened, resolve_stored = state_checks.flatten_app_state(
        app_state, save_dtype
    )
    found = _fingerprint_leaves(
        flattened, flattened.keys(), resolve_stored, True
    )
    return {path: f[0] for path, f in found.items()}
