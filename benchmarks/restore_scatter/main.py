#!/usr/bin/env python3
"""Device restore under each TSAMD_RESTORE_MODE.

  direct  one scatter kernel per read pulls the bytes out of pinned memory
  slab    one H2D copy into a device slab per read, then one scatter kernel
  torch   .to(device) of the payload + one copy_ per member

Two cases, both restored into device tensors from a warm page cache:

  small   2000 x 0.5 MB fp32 tensors (batched slabs: one span read each)
  widen   one fp32 state of --widen-gib saved as bf16, restored into fp32

A third case, kernel, takes storage out of the picture: one 1 GiB pinned
payload into one device tensor, `StagingEngine.scatter` under direct (at
several TSAMD_PACK_GRID caps) and slab against `.to(device)` + `copy_`,
plain bf16 and bf16 -> fp32, with and without the fused checksum, in GB/s
of payload bytes.

For each (case, mode) of the first two it reports the restore rate in GB/s
of TARGET bytes (median of --reps after --warmup, modes interleaved) and
the rise in
torch.cuda.max_memory_allocated across one restore, which is the transient
device memory the mode costs. Restored values are compared across modes.
"""

import os
import sys

sys.path.insert(
    0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
)

import argparse
import json
import shutil
import statistics
import time

GIB = 1024**3
MODES = ("direct", "slab", "torch")


def _summary(xs):
    return {
        "median": statistics.median(xs),
        "min": min(xs),
        "max": max(xs),
        "n": len(xs),
        "samples": [round(x, 3) for x in xs],
    }


def _run_case(name, src, make_out, save_kw, args) -> dict:
    import torch

    from torchsnapshot_amd import Snapshot

    path = os.path.join(args.work_dir, name)
    shutil.rmtree(path, ignore_errors=True)
    snap = Snapshot.take(path, {"sd": src}, **save_kw)
    out = make_out()
    target_bytes = sum(
        t.numel() * t.element_size() for t in out.values()
    )
    rates = {m: [] for m in MODES}
    rises = {m: [] for m in MODES}
    sums = {}
    for rep in range(args.warmup + args.reps):
        for mode in MODES:
            os.environ["TSAMD_RESTORE_MODE"] = mode
            for t in out.values():
                t.zero_()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.max_memory_allocated()
            t0 = time.monotonic()
            snap.restore({"sd": out})
            torch.cuda.synchronize()
            dt = time.monotonic() - t0
            rise = torch.cuda.max_memory_allocated() - before
            if rep >= args.warmup:
                rates[mode].append(target_bytes / dt / 1e9)
                rises[mode].append(rise)
            if rep == 0:
                sums[mode] = [
                    float(t.double().sum().item()) for t in out.values()
                ]
    os.environ.pop("TSAMD_RESTORE_MODE", None)
    shutil.rmtree(path, ignore_errors=True)
    result = {"case": name, "target_bytes": target_bytes, "modes": {}}
    for mode in MODES:
        assert sums[mode] == sums["torch"], f"{name}: {mode} restored other values"
        result["modes"][mode] = {
            "restore_GBps": _summary(rates[mode]),
            "max_memory_allocated_rise_bytes": max(rises[mode]),
        }
        r = result["modes"][mode]["restore_GBps"]
        print(
            f"{name:>6}/{mode:<6}: {r['median']:.1f} GB/s "
            f"[{r['min']:.1f}..{r['max']:.1f}]  HBM rise "
            f"{max(rises[mode]) / 2**20:.1f} MiB"
        )
    return result


def _run_kernel_case(args) -> dict:
    import torch

    from torchsnapshot_amd.ops import staging

    device = torch.device("cuda", 0)
    engine = staging.get_staging_engine(device)
    block = staging.get_pinned_pool().acquire(GIB)
    payload = block.tensor[:GIB]
    payload.random_(0, 256)
    expected = (int(staging._csnap.psum64_host(payload.numpy(), 0)), 0)
    dst = {
        "bf16": torch.zeros(GIB // 2, dtype=torch.bfloat16, device=device),
        "bf16->f32": torch.zeros(GIB // 2, dtype=torch.float32, device=device),
    }

    def rate(fn):
        xs = []
        for rep in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.monotonic()
            fn()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                xs.append(GIB / (time.monotonic() - t0) / 1e9)
        return _summary(xs)

    def torch_path(target):
        dev = payload.to(device, non_blocking=False)
        target.copy_(dev.view(torch.bfloat16))

    def scatter(target, psum=None):
        engine.scatter(block, GIB, [(target, torch.bfloat16, 0)], psum)

    rows = {}
    for name, target in dst.items():
        rows[f"torch {name}"] = rate(lambda: torch_path(target))
    for mode, grids in (("direct", (None, 128, 1024, 4096)), ("slab", (None,))):
        os.environ["TSAMD_RESTORE_MODE"] = mode
        for grid in grids:
            if grid is not None:
                os.environ["TSAMD_PACK_GRID"] = str(grid)
            for name, target in dst.items():
                key = f"{mode} {name}" + (f" grid={grid}" if grid else "")
                rows[key] = rate(lambda: scatter(target))
            os.environ.pop("TSAMD_PACK_GRID", None)
        rows[f"{mode} bf16->f32 + psum64"] = rate(
            lambda: scatter(dst["bf16->f32"], expected)
        )
    os.environ.pop("TSAMD_RESTORE_MODE", None)
    staging.get_pinned_pool().release(block)
    for key, r in rows.items():
        print(f"kernel/{key:<28}: {r['median']:.1f} GB/s [{r['min']:.1f}..{r['max']:.1f}]")
    return {"case": "kernel", "payload_bytes": GIB, "rows": rows}


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--work-dir", default="/tmp/tsamd_restore_scatter_bench")
    parser.add_argument("--widen-gib", type=float, default=4.0)
    parser.add_argument("--small-count", type=int, default=2000)
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=1)
    parser.add_argument(
        "--case", choices=["all", "small", "widen", "kernel"], default="all"
    )
    args = parser.parse_args()
    if args.case == "kernel":
        # its 1 GiB payload then comes out of the pinned pool; under "all"
        # the pool keeps its default blocks and the payload is a one-off
        os.environ.setdefault("TSAMD_PINNED_BLOCK_SIZE_BYTES", str(GIB))

    import torch

    from torchsnapshot_amd.state_dict import StateDict

    device = torch.device("cuda", 0)
    results = []
    if args.case in ("all", "small"):
        n = 500_000 // 4  # 0.5 MB fp32
        src = StateDict(
            **{
                f"t{i}": torch.randn(n, device=device)
                for i in range(args.small_count)
            }
        )
        results.append(
            _run_case(
                "small",
                src,
                lambda: StateDict(**{k: torch.zeros_like(v) for k, v in src.items()}),
                {},
                args,
            )
        )
        del src
    if args.case in ("all", "widen"):
        rows = max(int(args.widen_gib * GIB) // (4 * 4096), 1)
        src = StateDict(w=torch.randn(rows, 4096, device=device))
        results.append(
            _run_case(
                "widen",
                src,
                lambda: StateDict(w=torch.zeros_like(src["w"])),
                {"save_dtype": torch.bfloat16},
                args,
            )
        )
        del src
    if args.case in ("all", "kernel"):
        results.append(_run_kernel_case(args))
    shutil.rmtree(args.work_dir, ignore_errors=True)
    print(json.dumps({"benchmark": "restore_scatter", "cases": results}))


if __name__ == "__main__":
    main()
