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
from typing import Any, Callable, Dict, Iterable, List, Optional, Tuple

import torch

from . import knobs
from .flatten import flatten
from .integrity import format_psum64
from .pg_wrapper import PGWrapper
from .stateful import AppState

logger = logging.getLogger(__name__)

POLICIES = ("ignore", "warn", "error")

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
    if replicated_check is None:
        return knobs.get_replicated_check_policy()
    if replicated_check not in POLICIES:
        raise ValueError(
            f"replicated_check must be one of {'|'.join(POLICIES)} or None, "
            f"got {replicated_check!r}"
        )
    return replicated_check


def _local_tensor(obj: Any, dtensor_local: bool) -> Optional[torch.Tensor]:
    """The tensor to fingerprint behind one flattened leaf, or None: plain
    tensors and Parameters, and a DTensor's local shard when asked for."""
    if not isinstance(obj, torch.Tensor):
        return None
    try:
        from torch.distributed.tensor import DTensor

        if isinstance(obj, DTensor):
            return obj.to_local().detach() if dtensor_local else None
    except ImportError:
        pass
    if type(obj) is torch.Tensor or isinstance(obj, torch.nn.Parameter):
        return obj.detach()
    return None  # ShardedTensor and other subclasses


def _fingerprint_leaves(
    flattened: Dict[str, Any],
    paths: Iterable[str],
    resolve_stored: Callable[[str, Any], Optional[torch.dtype]],
    dtensor_local: bool,
) -> LocalReport:
    from .ops import staging

    # unique tensors to fingerprint, and which of them each path is
    keys: Dict[Any, int] = {}
    tensors: List[torch.Tensor] = []
    stored: List[Optional[torch.dtype]] = []
    member: Dict[str, int] = {}
    for path in sorted(paths):
        t = _local_tensor(flattened.get(path), dtensor_local)
        if t is None or t.device.type == "meta":
            continue
        stored_dtype = resolve_stored(path, flattened[path])
        key: Any = len(tensors)  # sparse: no data_ptr, never aliased
        if t.layout == torch.strided and not t.is_quantized:
            key = (
                t.data_ptr(),
                t.dtype,
                tuple(t.shape),
                tuple(t.stride()),
                str(t.device),
                t.is_conj(),
                t.is_neg(),
                stored_dtype,
            )
        if key not in keys:
            keys[key] = len(tensors)
            tensors.append(t)
            stored.append(stored_dtype)
        member[path] = keys[key]

    sums: List[int] = [0] * len(tensors)
    by_device: Dict[int, List[int]] = {}
    for i, t in enumerate(tensors):
        if t.device.type == "cuda":
            by_device.setdefault(t.device.index or 0, []).append(i)
        else:
            sums[i] = staging.host_fingerprint(t, stored[i])
    for dev_index, idxs in by_device.items():
        engine = staging.get_staging_engine(torch.device("cuda", dev_index))
        got = engine.fingerprint(
            [tensors[i] for i in idxs], [stored[i] for i in idxs]
        )
        for i, v in zip(idxs, got):
            sums[i] = v

    return {
        path: (
            format_psum64(sums[i]),
            str(stored[i] or tensors[i].dtype),
            tuple(tensors[i].shape),
        )
        for path, i in member.items()
    }


def fingerprint_leaves(
    flattened: Dict[str, Any],
    paths: Iterable[str],
    resolve_stored: Callable[[str, Any], Optional[torch.dtype]],
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
    world_size = pg_wrapper.get_world_size()
    gathered: List[Optional[LocalReport]] = [None] * world_size
    if world_size > 1:
        pg_wrapper.all_gather_object(gathered, local)
    else:
        gathered[0] = local
    found = [g or {} for g in gathered]
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
    from .snapshot import _normalize_save_dtype, _resolve_save_dtype

    rules = _normalize_save_dtype(save_dtype)
    flattened: Dict[str, Any] = {}
    for key, stateful in app_state.items():
        _, f = flatten(stateful.state_dict(), prefix=key)
        flattened.update(f)
    found = _fingerprint_leaves(
        flattened,
        flattened.keys(),
        lambda path, obj: _resolve_save_dtype(rules, path, obj),
        True,
    )
    return {path: f[0] for path, f in found.items()}
