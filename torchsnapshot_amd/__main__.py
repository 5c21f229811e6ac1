"""Snapshot inspection CLI.

    python -m torchsnapshot_amd inspect <path>       # manifest tree + sizes
    python -m torchsnapshot_amd cat <path> <entry>   # print one object
    python -m torchsnapshot_amd stats <path> [--against <other>]
                                                     # recorded statistics
    python -m torchsnapshot_amd hist <path> [<glob>] [--narrow <dtype>]
                                                     # exponent histograms
    python -m torchsnapshot_amd compare <path> <other>
                                                     # element-wise difference
"""

from __future__ import annotations

import argparse
import sys
from collections import defaultdict

from .manifest import (
    ChunkedTensorEntry,
    DTensorEntry,
    ObjectEntry,
    PrimitiveEntry,
    ShardedTensorEntry,
    TensorEntry,
    is_container_entry,
)
from .snapshot import Snapshot


def _entry_bytes(entry) -> int:
    if isinstance(entry, TensorEntry):
        return entry.nbytes_estimate()
    if isinstance(entry, ChunkedTensorEntry):
        return sum(c.tensor.nbytes_estimate() for c in entry.chunks)
    if isinstance(entry, (ShardedTensorEntry, DTensorEntry)):
        return sum(s.tensor.nbytes_estimate() for s in entry.shards)
    return 0


def _describe(entry) -> str:
    if isinstance(entry, TensorEntry):
        return f"tensor {entry.dtype}{entry.shape} -> {entry.location}"
    if isinstance(entry, ChunkedTensorEntry):
        return (
            f"chunked_tensor {entry.dtype}{entry.shape} "
            f"({len(entry.chunks)} chunks)"
        )
    if isinstance(entry, ShardedTensorEntry):
        return (
            f"sharded_tensor {entry.dtype}{entry.shape} "
            f"({len(entry.shards)} shards)"
        )
    if isinstance(entry, DTensorEntry):
        return (
            f"dtensor {entry.dtype}{entry.shape} mesh={entry.mesh} "
            f"dim_map={entry.dim_map}"
        )
    if isinstance(entry, ObjectEntry):
        return f"object ({entry.obj_type}) -> {entry.location}"
    if isinstance(entry, PrimitiveEntry):
        return f"primitive {entry.ptype} = {entry.get_value()!r}"
    return type(entry).__name__


def cmd_inspect(args: argparse.Namespace) -> int:
    snapshot = Snapshot(args.path)
    md = snapshot.metadata
    print(f"snapshot: {args.path}")
    print(f"version: {md.version}  world_size: {md.world_size}")
    per_rank_bytes: dict = defaultdict(int)
    n_payloads = 0
    for key, entry in sorted(md.manifest.items()):
        if is_container_entry(entry):
            continue
        rank = key.partition("/")[0]
        nbytes = _entry_bytes(entry)
        per_rank_bytes[rank] += nbytes
        n_payloads += 1
        if not args.summary:
            print(f"  {key}: {_describe(entry)} [{nbytes / 1e6:.2f} MB]")
    total = sum(per_rank_bytes.values())
    print(f"{n_payloads} payload entries, {total / 1e9:.3f} GB logical")
    for rank in sorted(per_rank_bytes, key=int):
        print(f"  rank {rank}: {per_rank_bytes[rank] / 1e9:.3f} GB")
    return 0


def cmd_cat(args: argparse.Namespace) -> int:
    snapshot = Snapshot(args.path)
    obj = snapshot.read_object(args.entry)
    print(obj)
    return 0


def _fmt(x) -> str:
    return "-" if x is None else f"{x:.6g}"


def cmd_stats(args: argparse.Namespace) -> int:
    from .tensor_stats import relative_change

    stats = Snapshot(args.path).get_stats()
    if not stats:
        print(f"{args.path}: no statistics recorded (take(..., stats=True))")
        return 1
    against = None
    if args.against is not None:
        against = Snapshot(args.against).get_stats()
    rows = []
    for path, s in stats.items():
        line = (
            f"{path}: n_finite={s.n_finite} n_zero={s.n_zero} "
            f"min={_fmt(s.min)} max={_fmt(s.max)} mean={_fmt(s.mean)} "
            f"rms={_fmt(s.rms)} absmax={_fmt(s.absmax)}"
        )
        change = -1.0
        if against is not None:
            old = against.get(path)
            d_rms = relative_change(s.rms, old.rms) if old else None
            d_abs = relative_change(s.absmax, old.absmax) if old else None
            line += f" d_rms={_fmt(d_rms)} d_absmax={_fmt(d_abs)}"
            change = max((d for d in (d_rms, d_abs) if d is not None), default=-1.0)
        rows.append((change, line))
    if against is not None:
        # the leaves that moved most first
        rows.sort(key=lambda r: -r[0])
    for _, line in rows:
        print(line)
    return 0


def cmd_compare(args: argparse.Namespace) -> int:
    """PATH against the tensors of OTHER, loaded to the host: one line per
    differing path, largest relative error first (paths without one last)."""
    from .state_dict import StateDict

    other = Snapshot(args.other)
    keys = sorted(
        {k.partition("/")[2].partition("/")[0] for k in other.metadata.manifest}
    )
    state = {k: StateDict(other.get_state_dict_for_key(k)) for k in keys if k}
    rows = []
    for path, d in Snapshot(args.path).compare(state).items():
        if d.equal:
            continue
        rel = d.rel_err if d.note is None else None
        line = f"{path}: " + (
            d.note
            if d.note is not None
            else f"n={d.n} n_diff={d.n_diff} n_nonfinite_diff={d.n_nonfinite_diff} "
            f"max_abs={_fmt(d.max_abs)} rms_err={_fmt(d.rms_err)} "
            f"rel_err={_fmt(rel)}"
        )
        rows.append((-1.0 if rel is None else rel, line))
    rows.sort(key=lambda r: -r[0])
    for _, line in rows:
        print(line)
    return 1 if rows else 0


_NARROW = ("float16", "bfloat16", "float8_e4m3fn", "float8_e5m2")


def cmd_hist(args: argparse.Namespace) -> int:
    import fnmatch

    import torch

    hists = Snapshot(args.path).get_histograms()
    if not hists:
        print(f"{args.path}: no histograms recorded (take(..., histogram=True))")
        return 1
    for path, h in hists.items():
        if args.glob is not None and not fnmatch.fnmatchcase(path, args.glob):
            continue
        lo, hi = h.exponent_range
        span = f"2^{lo}..2^{hi}" if h.bins else "-"
        line = (
            f"{path}: n={h.n} exponents={span} n_zero={h.n_zero} "
            f"n_negative={h.n_negative} n_nonfinite={h.n_nonfinite}"
        )
        if args.narrow is not None:
            over, flushed, sub = h.narrowing(getattr(torch, args.narrow))
            line += (
                f" {args.narrow}: overflow={over} flushed={flushed} "
                f"subnormal={sub}"
            )
        print(line)
    return 0


def main(argv=None) -> int:
    parser = argparse.ArgumentParser(prog="python -m torchsnapshot_amd")
    sub = parser.add_subparsers(dest="cmd", required=True)
    p_inspect = sub.add_parser("inspect", help="print the manifest tree")
    p_inspect.add_argument("path")
    p_inspect.add_argument("--summary", action="store_true")
    p_inspect.set_defaults(fn=cmd_inspect)
    p_cat = sub.add_parser("cat", help="print one object by manifest path")
    p_cat.add_argument("path")
    p_cat.add_argument("entry")
    p_cat.set_defaults(fn=cmd_cat)
    p_stats = sub.add_parser(
        "stats", help="print the statistics recorded by take(..., stats=True)"
    )
    p_stats.add_argument("path")
    p_stats.add_argument(
        "--against",
        metavar="OTHER",
        help="also print the relative change of rms and absmax since the "
        "snapshot at OTHER, largest first",
    )
    p_stats.set_defaults(fn=cmd_stats)
    p_compare = sub.add_parser(
        "compare", help="compare a snapshot with another, element by element"
    )
    p_compare.add_argument("path")
    p_compare.add_argument("other")
    p_compare.set_defaults(fn=cmd_compare)
    p_hist = sub.add_parser(
        "hist",
        help="print the exponent histograms recorded by take(..., histogram=True)",
    )
    p_hist.add_argument("path")
    p_hist.add_argument("glob", nargs="?", help="only leaves matching this glob")
    p_hist.add_argument(
        "--narrow",
        metavar="DTYPE",
        choices=sorted(_NARROW),
        help="also print how many elements a cast to DTYPE would turn into "
        "Inf, flush to zero or leave subnormal, by binade",
    )
    p_hist.set_defaults(fn=cmd_hist)
    args = parser.parse_args(argv)
    return args.fn(args)


if __name__ == "__main__":
    sys.exit(main())
