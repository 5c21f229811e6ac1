#!/usr/bin/env python3
"""Flagship benchmark: checkpoint-save throughput for an FSDP-sharded
Llama-3-8B (bf16, random-init, synthetic) written to local NVMe.

One "step" = one full Snapshot.take of the model state. The whole-job
metric is aggregate save GB/s (model bytes / wall time per save, maxed
over ranks). Also reports the async_take stall time (how long training is
blocked by a non-blocking snapshot).

Launch (driver contract):
    python bench.py --gpus 1 --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run does only what the headline figure needs: set up, warm up,
time the K saves, print the result line. ``--full`` adds the secondary
measurements (async_take stall, restore throughput), each of which takes
runs of its own. ``--dump-outputs DIR`` writes what the last timed save
put on disk, read back through Snapshot.read_object, as DIR/<name>.npy
(float32; tensors too large for the dump budget are stored as a fixed,
seeded sample of their elements). The synthetic state is seeded, so two
runs with the same arguments save identical values.

At every N (including 1) each rank holds 1/N of every parameter as a
DTensor on a 1-D mesh (FSDP2-style layout), so the FSDP write path named
by the metric is always the one timed; if the 1-rank process group can't
come up, N=1 falls back to plain device tensors (parallelism "single").
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import time
from typing import Dict, List, Optional, Tuple

import torch

# Reference baseline: implied GB/s of torchsnapshot's published 20 GB DDP
# save to local FS on p4d.24xlarge (1 GPU ~13.91 s, 8 GPUs
# ~3.38 s). 2/4-GPU points interpolated geometrically.
_BASELINE_GBPS = {1: 1.44, 2: 2.29, 4: 3.65, 8: 5.92}

_STATE_SEED = 20240531  # synthetic model state
_DUMP_SEED = 977  # element sample of --dump-outputs
# --dump-outputs writes at most this much (float32) across all tensors
_DUMP_BUDGET_BYTES = 48 * 1024 * 1024


def _default_bench_dir() -> str:
    """/tmp/tsamd_bench, or a per-user sibling when another user owns it."""
    path = "/tmp/tsamd_bench"
    if os.path.exists(path) and not os.access(path, os.W_OK | os.X_OK):
        path = f"{path}_{os.getuid()}"
    return path


def dump_outputs(ckpt_path: str, names: List[str], out_dir: str) -> None:
    """Write what the snapshot at ``ckpt_path`` stores for each tensor of
    the "model" state as ``out_dir/<name>.npy`` (float32).

    Every tensor is read back from storage in full (sharded ones are
    reassembled). Each gets an equal share of the dump budget; one that
    fits is written whole, a larger one as the elements at a sorted index
    sample drawn from a fixed seed, so two runs pick the same elements."""
    import numpy as np

    from torchsnapshot_amd import Snapshot

    os.makedirs(out_dir, exist_ok=True)
    snap = Snapshot(ckpt_path)
    cap = max(1, _DUMP_BUDGET_BYTES // 4 // max(1, len(names)))
    gen = torch.Generator().manual_seed(_DUMP_SEED)
    for name in names:
        t = snap.read_object(f"0/model/{name}")
        flat = t.detach().cpu().reshape(-1)
        if flat.numel() > cap:
            idx = torch.randint(flat.numel(), (cap,), generator=gen)
            flat = flat[idx.sort().values]
        np.save(
            os.path.join(out_dir, f"{name}.npy"),
            flat.to(torch.float32).numpy(),
        )


def tiny_shapes() -> List[Tuple[str, Tuple[int, ...]]]:
    """Miniature llama-shaped state for CPU smoke tests of the bench path."""
    return [
        ("embed.weight", (64, 16)),
        ("layer.wq.weight", (16, 16)),
        ("layer.norm.weight", (16,)),
        ("head.weight", (64, 16)),
    ]


def llama3_8b_shapes() -> List[Tuple[str, Tuple[int, ...]]]:
    """Parameter shapes of Llama-3-8B (vocab 128256, hidden 4096,
    intermediate 14336, 32 layers, 32 heads / 8 KV heads)."""
    V, H, I, L = 128256, 4096, 14336, 32
    KV = 1024  # 8 kv heads * 128 head_dim
    shapes: List[Tuple[str, Tuple[int, ...]]] = [
        ("model.embed_tokens.weight", (V, H)),
        ("model.norm.weight", (H,)),
        ("lm_head.weight", (V, H)),
    ]
    for i in range(L):
        p = f"model.layers.{i}"
        shapes += [
            (f"{p}.self_attn.q_proj.weight", (H, H)),
            (f"{p}.self_attn.k_proj.weight", (KV, H)),
            (f"{p}.self_attn.v_proj.weight", (KV, H)),
            (f"{p}.self_attn.o_proj.weight", (H, H)),
            (f"{p}.mlp.gate_proj.weight", (I, H)),
            (f"{p}.mlp.up_proj.weight", (I, H)),
            (f"{p}.mlp.down_proj.weight", (H, I)),
            (f"{p}.input_layernorm.weight", (H,)),
            (f"{p}.post_attention_layernorm.weight", (H,)),
        ]
    return shapes


class _BenchState:
    """Stateful wrapper over the synthetic model state dict."""

    def __init__(self, sd: Dict[str, torch.Tensor]) -> None:
        self._sd = sd

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return self._sd

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        self._sd = sd


def build_state(
    device: torch.device,
    world_size: int,
    dtype: torch.dtype,
    model: str = "llama3-8b",
    use_dtensor: Optional[bool] = None,
) -> Tuple[_BenchState, int]:
    if use_dtensor is None:
        use_dtensor = world_size > 1
    shapes = tiny_shapes() if model == "tiny" else llama3_8b_shapes()
    total_bytes = 0
    sd: Dict[str, torch.Tensor] = {}
    if use_dtensor:
        from torch.distributed.device_mesh import init_device_mesh
        from torch.distributed.tensor import DTensor
        from torch.distributed.tensor.placement_types import Shard

        mesh = init_device_mesh(device.type, (world_size,))
        rank = int(os.environ.get("RANK", "0"))
        for name, shape in shapes:
            # uneven Shard(0) split with torch.chunk semantics (what
            # DTensor uses): ceil-sized chunks, trailing ranks may hold
            # fewer (or zero) rows — no divisibility requirement
            chunk = -(-shape[0] // world_size)
            lo = min(rank * chunk, shape[0])
            hi = min(lo + chunk, shape[0])
            local_shape = (hi - lo,) + tuple(shape[1:])
            local = torch.empty(local_shape, dtype=dtype, device=device)
            if local.numel():
                local = local.float().normal_(0, 0.02).to(dtype)
            full_stride = torch.empty(
                shape, dtype=dtype, device="meta"
            ).stride()
            sd[name] = DTensor.from_local(
                local,
                mesh,
                [Shard(0)],
                run_check=False,
                shape=torch.Size(shape),
                stride=full_stride,
            )
            total_bytes += int(
                torch.Size(shape).numel() * local.element_size()
            )
    else:
        for name, shape in shapes:
            t = torch.empty(shape, dtype=dtype, device=device)
            t.normal_(0, 0.02)
            sd[name] = t
            total_bytes += t.numel() * t.element_size()
    return _BenchState(sd), total_bytes


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--gpus", type=int, default=1)
    parser.add_argument("--steps", type=int, default=3)
    parser.add_argument("--warmup", type=int, default=1)
    parser.add_argument(
        "--dir", type=str, default=os.environ.get("TSAMD_BENCH_DIR", "")
    )
    parser.add_argument(
        "--keep", action="store_true", help="keep the checkpoint directory"
    )
    parser.add_argument("--device", choices=["cuda", "cpu"], default="cuda")
    parser.add_argument(
        "--model", choices=["llama3-8b", "tiny"], default="llama3-8b"
    )
    parser.add_argument(
        "--full",
        action="store_true",
        help="also measure the async_take stall and restore throughput",
    )
    parser.add_argument(
        "--dump-outputs",
        type=str,
        default="",
        metavar="DIR",
        help="write what the last timed save stored as DIR/<name>.npy",
    )
    args = parser.parse_args()
    if args.steps < 1:
        parser.error("--steps must be at least 1")

    from torchsnapshot_amd import Snapshot

    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    use_cuda = args.device == "cuda"
    # rehearsal escape hatch for 1-GPU boxes: TSAMD_BENCH_SHARE_DEVICE=1
    # puts every rank on cuda:0 over gloo so the multi-rank DTensor save
    # path can be exercised before an 8-GPU node exists. The driver's
    # launch (no env set) is unaffected: N ranks, cuda:LOCAL_RANK, RCCL.
    share_device = os.environ.get("TSAMD_BENCH_SHARE_DEVICE", "0") not in (
        "0",
        "",
    )
    if share_device:
        local_rank = 0
    if world_size > 1:
        import torch.distributed as dist

        if use_cuda and not share_device:
            torch.cuda.set_device(local_rank)
            dist.init_process_group(
                backend="nccl", device_id=torch.device("cuda", local_rank)
            )
        else:
            dist.init_process_group(backend="gloo")
    if use_cuda:
        device = torch.device("cuda", local_rank)
        torch.cuda.set_device(device)
    else:
        device = torch.device("cpu")

    # at world 1, still run the FSDP/DTensor write path (the metric's
    # named parallelism) on a 1-rank mesh; fall back to plain tensors if
    # the single-rank process group cannot come up
    use_dtensor = world_size > 1
    single_rank_pg = False
    if world_size == 1 and args.model != "tiny":
        import torch.distributed as dist

        try:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29561")
            kwargs = {"device_id": device} if use_cuda else {}
            dist.init_process_group(
                backend="nccl" if use_cuda else "gloo",
                rank=0,
                world_size=1,
                **kwargs,
            )
            use_dtensor = True
            single_rank_pg = True
        except Exception:
            use_dtensor = False

    bench_dir = args.dir or _default_bench_dir()
    ckpt_path = os.path.join(bench_dir, "ckpt")
    if rank == 0:
        os.makedirs(bench_dir, exist_ok=True)
        shutil.rmtree(ckpt_path, ignore_errors=True)
    _barrier(world_size)

    # same arguments -> same synthetic state, run after run (per-rank
    # offset so shards differ across ranks)
    torch.manual_seed(_STATE_SEED + rank)
    state, total_bytes = build_state(
        device,
        world_size,
        torch.bfloat16,
        model=args.model,
        use_dtensor=use_dtensor,
    )
    app_state = {"model": state}

    # warmup (untimed): allocates pinned blocks, compiles nothing, warms
    # the fs dir cache
    for _ in range(args.warmup):
        Snapshot.take(ckpt_path, app_state)
    # drain the warmup's dirty pages so every timed step starts from the
    # same writeback state (work outside the timed region)
    os.sync()
    _barrier(world_size)
    if use_cuda:
        torch.cuda.synchronize(device)

    t0 = time.monotonic()
    for _ in range(args.steps):
        Snapshot.take(ckpt_path, app_state)
    if use_cuda:
        torch.cuda.synchronize(device)
    _barrier(world_size)
    elapsed = time.monotonic() - t0
    elapsed = _max_over_ranks(elapsed, world_size, device)

    ms_per_step = elapsed / args.steps * 1000.0
    gbps = (total_bytes / 1e9) / (elapsed / args.steps)

    if args.dump_outputs:
        if rank == 0:
            dump_outputs(ckpt_path, list(state.state_dict()), args.dump_outputs)
        _barrier(world_size)

    extras: Dict[str, float] = {}
    if args.full:
        # async_take stall: how long the "training thread" is blocked.
        # Drain the timed loop's writeback backlog first (untimed) so the
        # stall reflects the snapshot machinery, not 16 GB/step of dirty
        # pages flushing under the measurement's CPU.
        os.sync()
        _barrier(world_size)
        t0 = time.monotonic()
        pending = Snapshot.async_take(ckpt_path, app_state)
        stall_s = time.monotonic() - t0
        pending.wait()
        stall_s = _max_over_ranks(stall_s, world_size, device)

        # informational: one restore of the full state (reported as
        # restore_GBps)
        _barrier(world_size)
        t0 = time.monotonic()
        Snapshot(ckpt_path).restore({"model": state})
        restore_s = _max_over_ranks(
            time.monotonic() - t0, world_size, device
        )
        extras = {
            "stall_sec": round(stall_s, 3),
            "restore_GBps": round((total_bytes / 1e9) / restore_s, 3),
        }

    if rank == 0 and not args.keep:
        shutil.rmtree(ckpt_path, ignore_errors=True)

    if rank == 0:
        baseline = _BASELINE_GBPS.get(world_size)
        result = {
            "metric": "checkpoint_save_GBps",
            "value": round(gbps, 3),
            "unit": "GB/s",
            "n_gpus": world_size,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 1),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": round(gbps / baseline, 3) if baseline else None,
            "dtype": "bf16",
            "data": "synthetic",
            **extras,
            "config": {
                "model": "llama-3-8b" if args.model != "tiny" else "tiny",
                "model_bytes": total_bytes,
                "global_batch": None,
                "seq_len": None,
                "parallelism": f"fsdp{world_size}" if use_dtensor else "single",
                "storage": bench_dir,
            },
        }
        print(json.dumps(result))

    if world_size > 1 or single_rank_pg:
        import torch.distributed as dist

        dist.destroy_process_group()


def _barrier(world_size: int) -> None:
    if world_size > 1:
        import torch.distributed as dist

        dist.barrier()


def _max_over_ranks(value: float, world_size: int, device) -> float:
    if world_size <= 1:
        return value
    import torch.distributed as dist

    dev = device if device.type == "cuda" else torch.device("cpu")
    t = torch.tensor([value], dtype=torch.float64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


if __name__ == "__main__":
    main()
