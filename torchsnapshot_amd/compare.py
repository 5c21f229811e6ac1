"""Compare a snapshot with live state, element by element.

``Snapshot.compare(app_state)`` drives restore's read pipeline with a compare
action on its consumers: where a consumer would scatter or copy a payload
into its target, it compares the two and adds the six fields to a
CompareSink. Device targets are compared by the compare kernel
(ops/hip/staging.hip) straight out of the pinned block the read landed in;
host targets, and whatever the kernel declines, by
``ops.staging.torch_tensor_diff``. Nothing is written to the state or under
the snapshot path.
"""

from __future__ import annotations

import math
import threading
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

from .io_types import ReadReq
from .ops.staging import merge_diff


@dataclass(frozen=True)
class TensorDiff:
    """One leaf of a snapshot against the live tensor. ``s`` is the stored
    element brought to the live dtype, ``v`` the live one. ``max_abs``,
    ``sum_sq`` (of v - s) and ``ref_sum_sq`` (of s) are float64 over the
    pairs with both sides finite, and None for dtypes that are compared
    bitwise only (integers, bool, fp8, complex). ``note`` says why a leaf was
    not compared; ``n`` is then 0."""

    n: int = 0
    n_diff: int = 0
    n_nonfinite_diff: int = 0
    max_abs: Optional[float] = None
    sum_sq: Optional[float] = None
    ref_sum_sq: Optional[float] = None
    note: Optional[str] = None

    @property
    def equal(self) -> bool:
        return self.n_diff == 0 and self.note is None

    @property
    def rms_err(self) -> Optional[float]:
        if self.sum_sq is None or self.n == 0:
            return None
        return math.sqrt(self.sum_sq / self.n)

    @property
    def rel_err(self) -> Optional[float]:
        if self.sum_sq is None or not self.ref_sum_sq:
            return None
        return math.sqrt(self.sum_sq / self.ref_sum_sq)


class CompareSink:
    """Per-path accumulator of a compare run. Consumers add the fields of
    the pieces they compared, from any thread and in any order; result()
    merges the pieces of a path in ascending key order, so the float64 sums
    do not depend on the order in which the reads completed."""

    def __init__(self) -> None:
        self._lock = threading.Lock()
        self._pieces: Dict[str, List[Tuple[Any, List[Any]]]] = {}
        self._notes: Dict[str, str] = {}

    def add(self, path: str, key: Any, fields: Sequence[Any]) -> None:
        with self._lock:
            self._pieces.setdefault(path, []).append((key, list(fields)))

    def note(self, path: str, text: str) -> None:
        self._notes[path] = text

    def result(self) -> Dict[str, TensorDiff]:
        out = {path: TensorDiff(note=text) for path, text in self._notes.items()}
        for path, pieces in self._pieces.items():
            # two pieces under one key (two views over one stored run) are
            # ordered by what they found, never by arrival
            pieces.sort(key=lambda p: (p[0], repr(p[1])))
            fields = pieces[0][1]
            for _, more in pieces[1:]:
                fields = merge_diff(fields, more)
            out[path] = TensorDiff(*fields)
        return dict(sorted(out.items()))


@dataclass
class CompareAction:
    """What a read consumer does instead of writing its target: ``add`` the
    fields of each piece it compared, keyed by the piece's place in the
    stored tensor (``key``, then the offset inside the payload)."""

    sink: CompareSink
    path: str
    key: Tuple[int, ...] = ()

    def add(self, offset: int, fields: Sequence[Any]) -> None:
        self.sink.add(self.path, (self.key, offset), fields)


def attach_compare(
    read_reqs: Sequence[ReadReq], sink: CompareSink, path: str, entry: Any = None
) -> None:
    """Give every consumer of ``read_reqs`` (one logical path's reads, before
    they are batched into spans) the compare action. ``entry`` is the path's
    manifest entry: the chunks or shards of one are keyed by their offsets
    in the stored tensor."""
    pieces = getattr(entry, "chunks", None) or getattr(entry, "shards", None) or ()
    keys = {id(p.tensor): tuple(p.offsets) for p in pieces}
    for rr in read_reqs:
        consumer = rr.consumer
        piece_entry = getattr(consumer, "entry", None) or getattr(
            consumer, "shard_entry", None
        )
        if not hasattr(consumer, "compare_members"):
            # tile and object consumers: compare plans neither
            raise TypeError(
                f"{type(consumer).__name__} has no compare action ({path})"
            )
        consumer.compare = CompareAction(sink, path, keys.get(id(piece_entry), ()))
