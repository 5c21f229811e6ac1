"""What the checks that read state before a snapshot share (nonfinite.py,
replication.py).

Both run at the same point of take(): before anything under the snapshot
path has been touched, each rank reads its state where it lies (device
tensors of one device by ONE kernel launch, host tensors on the CPU), one
all_gather_object exchanges a small report, and every rank applies the same
``ignore|warn|error`` policy. Here is that frame; which leaves a check looks
at, what it reports and how it decides stay with the check.
"""

from __future__ import annotations

import importlib
from typing import Any, Callable, Dict, List, Optional, Tuple

import torch

from .flatten import flatten
from .pg_wrapper import PGWrapper
from .serialization import is_mx
from .stateful import AppState

POLICIES = ("ignore", "warn", "error")

# names the dtype a leaf will be stored as (None = its own)
ResolveStored = Callable[[str, Any], Optional[torch.dtype]]


def resolve_policy(
    value: Optional[str], name: str, knob: Callable[[], str]
) -> str:
    """The policy of one take() call: its ``name`` argument, or the knob
    when that is None. Anything else raises ValueError."""
    if value is None:
        return knob()
    if value not in POLICIES:
        raise ValueError(
            f"{name} must be one of {'|'.join(POLICIES)} or None, "
            f"got {value!r}"
        )
    return value


def _optional_class(module: str, name: str) -> Any:
    """A class of torch.distributed, or ``()`` (of which nothing is an
    instance) in a torch build without it."""
    try:
        return getattr(importlib.import_module(module), name)
    except ImportError:
        return ()


def is_dtensor(obj: Any) -> bool:
    return isinstance(obj, _optional_class("torch.distributed.tensor", "DTensor"))


def is_sharded_tensor(obj: Any) -> bool:
    return isinstance(
        obj,
        _optional_class("torch.distributed._shard.sharded_tensor", "ShardedTensor"),
    )


def is_plain_tensor(obj: Any) -> bool:
    """A torch.Tensor proper or a Parameter, no other subclass."""
    return type(obj) is torch.Tensor or isinstance(obj, torch.nn.Parameter)


class UniqueTensors:
    """The tensors one check reads, each aliased tensor (tied weights) once:
    ``add`` returns an index into ``tensors`` / ``stored``, the same one for
    the same memory, layout, lazy bits and stored dtype."""

    def __init__(self) -> None:
        self._index: Dict[Any, int] = {}
        self.tensors: List[torch.Tensor] = []
        self.stored: List[Optional[torch.dtype]] = []

    def add(self, t: torch.Tensor, stored_dtype: Optional[torch.dtype]) -> int:
        if is_mx(stored_dtype):
            # the checks read live values under a block-scaled format:
            # quantising creates no Inf, and replicas are compared by their
            # live bytes
            stored_dtype = None
        key: Any = len(self.tensors)  # sparse: no data_ptr, never aliased
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
        if key not in self._index:
            self._index[key] = len(self.tensors)
            self.tensors.append(t)
            self.stored.append(stored_dtype)
        return self._index[key]

    def read(self, host_fn: str, engine_method: str) -> List[Any]:
        """One result per tensor: ``staging.<host_fn>(tensor, stored)`` for a
        host tensor, and for the device tensors of each device ONE call of
        its StagingEngine's ``engine_method(tensors, stored)``."""
        from .ops import staging

        out: List[Any] = [None] * len(self.tensors)
        by_device: Dict[int, List[int]] = {}
        for i, t in enumerate(self.tensors):
            if t.device.type == "cuda":
                by_device.setdefault(t.device.index or 0, []).append(i)
            else:
                out[i] = getattr(staging, host_fn)(t, self.stored[i])
        for dev_index, idxs in by_device.items():
            engine = staging.get_staging_engine(torch.device("cuda", dev_index))
            got = getattr(engine, engine_method)(
                [self.tensors[i] for i in idxs], [self.stored[i] for i in idxs]
            )
            for i, v in zip(idxs, got):
                out[i] = v
        return out


def exchange(local: Dict[str, Any], pg_wrapper: PGWrapper) -> List[Dict[str, Any]]:
    """Every rank's report, by rank: one all_gather_object when there is
    more than one rank."""
    world_size = pg_wrapper.get_world_size()
    if world_size == 1:
        return [local]
    gathered: List[Optional[Dict[str, Any]]] = [None] * world_size
    pg_wrapper.all_gather_object(gathered, local)
    return [g or {} for g in gathered]


def flatten_app_state(
    app_state: AppState, save_dtype: Any
) -> Tuple[Dict[str, Any], ResolveStored]:
    """Every stateful's leaves by logical path, as take() flattens them, and
    the stored-dtype resolver of ``save_dtype`` (as for take)."""
    # snapshot imports the checks, which import this module
    from .snapshot import _normalize_save_dtype, _resolve_save_dtype

    rules = _normalize_save_dtype(save_dtype)
    flattened: Dict[str, Any] = {}
    for key, stateful in app_state.items():
        _, f = flatten(stateful.state_dict(), prefix=key)
        flattened.update(f)
    return flattened, lambda path, obj: _resolve_save_dtype(rules, path, obj)
