#!/usr/bin/env python3
"""Narrowing saves: fp32 device state written as bf16, three ways.

  fp32        plain save, nothing narrowed (context)
  hook        _custom_tensor_prepare_func=lambda p, t: t.to(torch.bfloat16)
              — one torch cast kernel per tensor on the caller's stream,
              a half-size device copy of the state, then the usual staging
  save_dtype  save_dtype=torch.bfloat16 — the cast runs inside the staging
              gather kernel on the side stream

Part "save" reports the wall time of Snapshot.take and the stall of
Snapshot.async_take for each (median of --reps after --warmup, variants
interleaved so disk state drifts hit all three alike). Part "stage" reports
the stage-only rate of engine.stage + wait on a 1 GiB fp32 tensor, cast vs
uncast, direct vs slab mode, in SOURCE bytes per second.

Each part runs in a fresh child process: the stage part sizes the pinned
pool's blocks to hold 1 GiB so no run pays a one-off pinned allocation.
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
import subprocess
import time

GIB = 1024**3
MIB = 1024**2


def _summary(xs):
    return {
        "median": statistics.median(xs),
        "min": min(xs),
        "max": max(xs),
        "n": len(xs),
        "samples": [round(x, 6) for x in xs],
    }


def part_save(args) -> dict:
    import torch

    from torchsnapshot_amd import Snapshot
    from torchsnapshot_amd.state_dict import StateDict

    device = torch.device("cuda", 0)
    per = 64 * MIB // 4  # 64 MiB fp32 per tensor
    n_tensors = max(int(args.state_gib * GIB) // (64 * MIB), 1)
    sd = StateDict(
        **{
            f"w{i}": torch.randn(per, dtype=torch.float32, device=device)
            for i in range(n_tensors)
        }
    )
    src_bytes = n_tensors * 64 * MIB
    variants = {
        "fp32": {},
        "hook": {
            "_custom_tensor_prepare_func": lambda p, t: t.to(torch.bfloat16)
        },
        "save_dtype": {"save_dtype": torch.bfloat16},
    }
    take_s = {k: [] for k in variants}
    stall_s = {k: [] for k in variants}
    async_total_s = {k: [] for k in variants}
    path = os.path.join(args.work_dir, "snap")
    for rep in range(args.warmup + args.reps):
        for name, kw in variants.items():
            shutil.rmtree(args.work_dir, ignore_errors=True)
            torch.cuda.synchronize()
            t0 = time.monotonic()
            Snapshot.take(path, {"sd": sd}, **kw)
            dt_take = time.monotonic() - t0

            shutil.rmtree(args.work_dir, ignore_errors=True)
            torch.cuda.synchronize()
            t0 = time.monotonic()
            pending = Snapshot.async_take(path, {"sd": sd}, **kw)
            dt_stall = time.monotonic() - t0
            pending.wait()
            dt_total = time.monotonic() - t0
            if rep >= args.warmup:
                take_s[name].append(dt_take)
                stall_s[name].append(dt_stall)
                async_total_s[name].append(dt_total)
    shutil.rmtree(args.work_dir, ignore_errors=True)
    out = {"part": "save", "source_bytes": src_bytes, "variants": {}}
    for name in variants:
        out["variants"][name] = {
            "take_s": _summary(take_s[name]),
            "async_stall_s": _summary(stall_s[name]),
            "async_total_s": _summary(async_total_s[name]),
        }
        t, s = out["variants"][name]["take_s"], out["variants"][name]["async_stall_s"]
        print(
            f"{name:>10}: take {t['median']:.3f}s [{t['min']:.3f}..{t['max']:.3f}]"
            f"  async stall {s['median'] * 1e3:.1f}ms "
            f"[{s['min'] * 1e3:.1f}..{s['max'] * 1e3:.1f}]"
        )
    return out


def part_stage(args) -> dict:
    import torch

    from torchsnapshot_amd.ops import staging

    device = torch.device("cuda", 0)
    n = GIB // 4
    t = torch.randn(n, dtype=torch.float32, device=device)
    halves = [t[: n // 2], t[n // 2 :]]
    engine = staging.get_staging_engine(device)
    cases = {
        # a single contiguous uncast tensor takes the SDMA copy, no kernel
        "uncast_sdma": ([t], None),
        "uncast_kernel": (halves, None),
        "cast_kernel": (halves, [torch.bfloat16, torch.bfloat16]),
        "cast_kernel_single": ([t], [torch.bfloat16]),
    }
    out = {"part": "stage", "source_bytes": GIB, "cases": {}}
    for mode in ("direct", "slab"):
        os.environ["TSAMD_STAGE_MODE"] = mode
        for name, (tensors, outs) in cases.items():
            rates = []
            for rep in range(args.warmup + args.reps):
                torch.cuda.synchronize()
                t0 = time.monotonic()
                batch = engine.stage(tensors, out_dtypes=outs)
                batch.wait()
                dt = time.monotonic() - t0
                batch.release()
                if rep >= args.warmup:
                    rates.append(GIB / dt / 1e9)
            out["cases"][f"{mode}/{name}"] = _summary(rates)
            r = out["cases"][f"{mode}/{name}"]
            print(
                f"{mode:>6}/{name:<18}: {r['median']:.1f} GB/s of source "
                f"[{r['min']:.1f}..{r['max']:.1f}]"
            )
    return out


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--work-dir", default="/tmp/tsamd_cast_save_bench")
    parser.add_argument("--state-gib", type=float, default=4.0)
    parser.add_argument("--reps", type=int, default=5)
    parser.add_argument("--warmup", type=int, default=2)
    parser.add_argument("--part", choices=["all", "save", "stage"], default="all")
    args = parser.parse_args()

    if args.part == "all":
        # fresh child per part; this parent never opens the GPU
        for part in ("stage", "save"):
            cmd = [
                sys.executable, os.path.abspath(__file__),
                "--work-dir", args.work_dir,
                "--state-gib", str(args.state_gib),
                "--reps", str(args.reps),
                "--warmup", str(args.warmup),
                "--part", part,
            ]
            subprocess.run(cmd, check=True)
        return
    if args.part == "stage":
        os.environ.setdefault(
            "TSAMD_PINNED_BLOCK_SIZE_BYTES", str(GIB + 4096)
        )
        result = part_stage(args)
    else:
        result = part_save(args)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
