"""DTensor preparer: sharded + (partially) replicated tensors on device
meshes (FSDP2 / HSDP / TP / SP layouts).

Write: each rank computes its local shard's global coordinates; within a
replica set (ranks holding identical shards) exactly one member writes each
payload, chosen round-robin by sub-shard index so replicated write load
spreads across the set (the reference routes this through its partitioner,
torchsnapshot/partitioner.py:90-104; here the choice is deterministic from
the mesh, saving a collective). All replicas emit identical entries; the
load-side merge dedups them by offsets (manifest_ops).

Read: the same overlap machinery as ShardedTensor, against
``obj_out.to_local()``. Parity with reference torchsnapshot/io_preparers/
dtensor.py:63-278.
"""

from __future__ import annotations

import contextlib
import copy
import logging
import threading
from typing import Any, Dict, Iterator, List, Optional, Tuple

import torch

from .. import knobs
from ..io_types import ReadReq, WriteReq
from ..manifest import DTensorEntry, Shard as ShardMeta
from ..serialization import dtype_to_str, str_to_dtype
from .sharded_tensor import (
    location_for_shard,
    plan_shard_reads,
    subdivide_shard,
)
from .tensor import LoadFuture, TensorIOPreparer

logger = logging.getLogger(__name__)


class _PlanMemo:
    """What the DTensors of one take share. A model's parameters sit on one
    or two meshes with a handful of distinct (placements, shape) pairs, and
    ``DeviceMesh.mesh`` alone rebuilds a tensor on every access. Keys use
    the mesh object's identity; the object is held in the value, so an id
    cannot be reused while the memo lives."""

    def __init__(self) -> None:
        # id(device_mesh) -> (device_mesh, mesh tensor, mesh as nested list)
        self.meshes: Dict[int, Tuple[Any, torch.Tensor, list]] = {}
        # (id(device_mesh), placements) -> sorted replica set
        self.replica_sets: Dict[Any, List[int]] = {}
        # (id(device_mesh), placements, shape) ->
        #     (local shape, global offset, dim map)
        self.layouts: Dict[Any, Tuple[List[int], List[int], List[List[int]]]] = {}


_plan_state = threading.local()


@contextlib.contextmanager
def planning_memo() -> Iterator[None]:
    """Scope of one take's planning loop: inside it, prepare_write computes
    what depends only on the mesh once per mesh, and what depends only on
    (mesh, placements, global shape) once per distinct triple. The entries
    it returns are the ones it returns outside the scope."""
    prev = getattr(_plan_state, "memo", None)
    _plan_state.memo = prev if prev is not None else _PlanMemo()
    try:
        yield
    finally:
        _plan_state.memo = prev


def _memo_mesh(memo: _PlanMemo, device_mesh: Any) -> Tuple[Any, torch.Tensor, list]:
    hit = memo.meshes.get(id(device_mesh))
    if hit is None:
        mesh = device_mesh.mesh
        hit = memo.meshes[id(device_mesh)] = (device_mesh, mesh, mesh.tolist())
    return hit


def _mesh_tensor(dt: Any) -> torch.Tensor:
    """The mesh tensor of the DTensor's device mesh."""
    memo = getattr(_plan_state, "memo", None)
    if memo is None:
        return dt.device_mesh.mesh
    return _memo_mesh(memo, dt.device_mesh)[1]


def _mesh_list(dt: Any) -> list:
    """The mesh as a nested list, as a manifest entry stores it."""
    memo = getattr(_plan_state, "memo", None)
    if memo is None:
        return dt.device_mesh.mesh.tolist()
    # a list of its own per entry: the manifest writer must not see one
    # object shared between entries
    return copy.deepcopy(_memo_mesh(memo, dt.device_mesh)[2])


def _dim_map(dt: Any) -> List[List[int]]:
    from torch.distributed.tensor.placement_types import Shard

    dim_map: List[List[int]] = [[] for _ in range(dt.ndim)]
    for mesh_dim, placement in enumerate(dt.placements):
        if isinstance(placement, Shard):
            dim_map[placement.dim].append(mesh_dim)
    return dim_map


def _local_global_offset(dt: Any) -> Tuple[List[int], List[int]]:
    """(local shape, global offset) of this rank's shard of the DTensor."""
    from torch.distributed.tensor._utils import (
        compute_local_shape_and_global_offset,
    )

    local_shape, global_offset = compute_local_shape_and_global_offset(
        dt.shape, dt.device_mesh, dt.placements
    )
    return list(local_shape), list(global_offset)


def _layout_of(dt: Any) -> Tuple[List[int], List[int], List[List[int]]]:
    """(local shape, global offset, dim map): functions of the mesh, the
    placements and the global shape alone."""
    memo = getattr(_plan_state, "memo", None)
    if memo is None:
        return (*_local_global_offset(dt), _dim_map(dt))
    key = (id(dt.device_mesh), tuple(dt.placements), tuple(dt.shape))
    hit = memo.layouts.get(key)
    if hit is None:
        _memo_mesh(memo, dt.device_mesh)  # holds the mesh object: see _PlanMemo
        hit = memo.layouts[key] = (*_local_global_offset(dt), _dim_map(dt))
    return list(hit[0]), list(hit[1]), [list(d) for d in hit[2]]


def _my_replica_set(dt: Any) -> List[int]:
    """Global ranks that hold a shard identical to this rank's (the ranks
    reached by varying only replicated mesh dims at this rank's mesh
    coordinate). Inside a take it is computed once per (mesh, placements):
    a model checkpoint asks once per parameter with identical inputs, and
    the mesh tensor math is measurable in the async-stall window under CPU
    contention."""
    memo = getattr(_plan_state, "memo", None)
    if memo is None:
        return _my_replica_set_impl(dt)
    key = (id(dt.device_mesh), tuple(dt.placements))
    hit = memo.replica_sets.get(key)
    if hit is None:
        _memo_mesh(memo, dt.device_mesh)
        hit = memo.replica_sets[key] = _my_replica_set_impl(dt)
    return list(hit)


def _my_replica_set_impl(dt: Any) -> List[int]:
    from torch.distributed.tensor.placement_types import Shard

    mesh = _mesh_tensor(dt)
    sharded_mesh_dims = {
        mesh_dim
        for mesh_dim, p in enumerate(dt.placements)
        if isinstance(p, Shard)
    }
    rank = torch.distributed.get_rank() if torch.distributed.is_initialized() else 0
    coord = (mesh == rank).nonzero()
    if coord.numel() == 0:
        return [rank]
    coord = coord[0].tolist()
    # vary replicated dims, fix sharded dims
    index: List[Any] = []
    for d in range(mesh.dim()):
        if d in sharded_mesh_dims:
            index.append(coord[d])
        else:
            index.append(slice(None))
    subset = mesh[tuple(index)]
    return [int(r) for r in subset.flatten().tolist()]


class DTensorIOPreparer:
    @staticmethod
    def prepare_write(
        storage_path: str,
        obj: Any,  # DTensor
        is_async_snapshot: bool = False,
        save_dtype: Optional[torch.dtype] = None,
    ) -> Tuple[DTensorEntry, List[WriteReq]]:
        local = obj.to_local()
        local_shape, global_offset, dim_map = _layout_of(obj)
        if list(local.shape) != local_shape:
            # padded uneven shard (torch pads the last rank): trim
            local = local[tuple(slice(0, s) for s in local_shape)]

        replica_set = sorted(_my_replica_set(obj))
        my_rank = (
            torch.distributed.get_rank()
            if torch.distributed.is_initialized()
            else 0
        )
        max_bytes = knobs.get_max_shard_size_bytes()

        shards_meta: List[ShardMeta] = []
        write_reqs: List[WriteReq] = []
        pieces = subdivide_shard(local, global_offset, max_bytes)
        for i, (piece, piece_offsets) in enumerate(pieces):
            # round-robin writer within the replica set. ONLY the writer
            # emits the shard entry: non-writer copies would keep the
            # standalone location after the writer's batcher relocates the
            # payload into a slab, and the load-side merge could pick the
            # stale copy (round-1 advisor finding). The load-side merge
            # unions shards across all ranks, so readers still see the
            # full shard set.
            writer = replica_set[i % len(replica_set)]
            if writer != my_rank:
                continue
            location = location_for_shard(storage_path, piece_offsets)
            sub_entry, sub_reqs = TensorIOPreparer.prepare_write(
                storage_path=location,
                tensor=piece,
                replicated=False,
                is_async_snapshot=is_async_snapshot,
                save_dtype=save_dtype,
            )
            shards_meta.append(
                ShardMeta(
                    offsets=piece_offsets,
                    sizes=list(piece.shape),
                    tensor=sub_entry,
                )
            )
            write_reqs.extend(sub_reqs)
        entry = DTensorEntry(
            shards=shards_meta,
            mesh=_mesh_list(obj),
            dim_map=dim_map,
            dtype=dtype_to_str(save_dtype or obj.dtype),
            shape=list(obj.shape),
        )
        return entry, write_reqs

    @staticmethod
    def prepare_read(
        entry: DTensorEntry,
        obj_out: Optional[Any] = None,
    ) -> Tuple[List[ReadReq], LoadFuture]:
        try:
            from torch.distributed.tensor import DTensor
        except ImportError:
            DTensor = ()  # type: ignore[assignment]

        if isinstance(obj_out, DTensor):
            local = obj_out.to_local()
            local_shape, global_offset = _local_global_offset(obj_out)
            if list(local.shape) != local_shape:
                local = local[tuple(slice(0, s) for s in local_shape)]
            targets = [(local, global_offset)]
            fut = LoadFuture(obj_out)
            return plan_shard_reads(entry.shards, targets), fut

        if isinstance(obj_out, torch.Tensor):
            full = obj_out
        else:
            full = torch.empty(entry.shape, dtype=str_to_dtype(entry.dtype))
        targets = [(full, [0] * full.dim())]
        fut = LoadFuture(full)
        return plan_shard_reads(entry.shards, targets), fut
