"""Smoke the bench pipeline on CPU: tiny model, world 1 and world 2
(gloo), exactly the code path the driver exercises on the GPU node."""

import json
import os
import subprocess
import sys
import tempfile

import pytest

pytestmark = pytest.mark.timeout(300)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    return subprocess.run(
        cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=240
    )


def test_bench_tiny_single():
    with tempfile.TemporaryDirectory() as d:
        r = _run(
            [
                sys.executable,
                "bench.py",
                "--device",
                "cpu",
                "--model",
                "tiny",
                "--steps",
                "2",
                "--warmup",
                "1",
                "--dir",
                d,
                "--full",
            ]
        )
        assert r.returncode == 0, r.stderr[-2000:]
        line = r.stdout.strip().splitlines()[-1]
        out = json.loads(line)
        assert out["metric"] == "checkpoint_save_GBps"
        assert out["n_gpus"] == 1
        assert out["ms_per_step"] > 0
        assert out["stall_sec"] >= 0
        assert out["restore_GBps"] > 0


def test_bench_tiny_plain_and_dump_outputs():
    """A plain run prints the headline keys without the --full extras, and
    --dump-outputs writes the saved tensors, identical from run to run."""
    import importlib.util

    import numpy as np

    spec = importlib.util.spec_from_file_location(
        "_bench_under_test", os.path.join(REPO, "bench.py")
    )
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    shapes = dict(bench.tiny_shapes())
    dumps = []
    with tempfile.TemporaryDirectory() as d:
        for i in range(2):
            dump_dir = os.path.join(d, f"dump{i}")
            r = _run(
                [
                    sys.executable,
                    "bench.py",
                    "--device",
                    "cpu",
                    "--model",
                    "tiny",
                    "--steps",
                    "2",
                    "--warmup",
                    "0",
                    "--dir",
                    os.path.join(d, "ckpt"),
                    "--dump-outputs",
                    dump_dir,
                ]
            )
            assert r.returncode == 0, r.stderr[-2000:]
            out = json.loads(r.stdout.strip().splitlines()[-1])
            assert out["metric"] == "checkpoint_save_GBps"
            assert out["value"] >= 0 and out["unit"] == "GB/s"
            assert out["higher_is_better"] is True and out["dtype"] == "bf16"
            assert out["steps"] == 2
            assert out["ms_per_step"] > 0
            assert "stall_sec" not in out and "restore_GBps" not in out
            assert sorted(os.listdir(dump_dir)) == sorted(
                f"{name}.npy" for name in shapes
            )
            dumps.append(
                {
                    name: np.load(os.path.join(dump_dir, f"{name}.npy"))
                    for name in shapes
                }
            )
    for name, shape in shapes.items():
        a, b = dumps[0][name], dumps[1][name]
        assert a.dtype == np.float32
        assert a.size == int(np.prod(shape))
        assert np.isfinite(a).all() and a.std() > 0
        assert np.array_equal(a, b)


def test_dump_outputs_samples_large_tensors(monkeypatch):
    """A tensor over its share of the dump budget is written as a fixed
    sorted sample of the stored elements; a small one is written whole."""
    import importlib.util

    import numpy as np
    import torch

    from torchsnapshot_amd import Snapshot

    spec = importlib.util.spec_from_file_location(
        "_bench_under_test", os.path.join(REPO, "bench.py")
    )
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    # 2 tensors share 800 bytes -> 100 float32 elements each
    monkeypatch.setattr(bench, "_DUMP_BUDGET_BYTES", 800)
    torch.manual_seed(5)
    sd = {
        "big": torch.randn(37, 29).to(torch.bfloat16),
        "small": torch.randn(7).to(torch.bfloat16),
    }
    with tempfile.TemporaryDirectory() as d:
        ckpt = os.path.join(d, "ckpt")
        Snapshot.take(ckpt, {"model": bench._BenchState(sd)})
        outs = []
        for i in range(2):
            out_dir = os.path.join(d, f"dump{i}")
            bench.dump_outputs(ckpt, list(sd), out_dir)
            outs.append(
                {k: np.load(os.path.join(out_dir, f"{k}.npy")) for k in sd}
            )
    small = sd["small"].float().numpy()
    assert np.array_equal(outs[0]["small"], small)
    big = outs[0]["big"]
    assert big.dtype == np.float32 and big.shape == (100,)
    assert np.array_equal(big, outs[1]["big"])
    # every sampled value is a stored value, and the sample is spread out
    stored = sd["big"].float().numpy().reshape(-1)
    assert np.isin(big, stored).all()
    assert len(np.unique(big)) > 50


def test_bench_tiny_world2_gloo():
    with tempfile.TemporaryDirectory() as d:
        r = _run(
            [
                sys.executable,
                "-m",
                "torch.distributed.run",
                "--nnodes=1",
                "--nproc-per-node",
                "2",
                "--master-addr",
                "127.0.0.1",
                "--master-port",
                "29511",
                "bench.py",
                "--device",
                "cpu",
                "--model",
                "tiny",
                "--steps",
                "2",
                "--warmup",
                "1",
                "--dir",
                d,
            ]
        )
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
        lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
        out = json.loads(lines[-1])
        assert out["n_gpus"] == 2
        assert out["config"]["parallelism"] == "fsdp2"
        assert out["ms_per_step"] > 0


def test_bench_tiny_world3_uneven_gloo():
    """World 3 makes every tiny shape split unevenly (64 -> 22/22/20,
    16 -> 6/6/4): the bench (and the DTensor save path under it) must not
    require divisible shards."""
    with tempfile.TemporaryDirectory() as d:
        r = _run(
            [
                sys.executable,
                "-m",
                "torch.distributed.run",
                "--nnodes=1",
                "--nproc-per-node",
                "3",
                "--master-addr",
                "127.0.0.1",
                "--master-port",
                "29513",
                "bench.py",
                "--device",
                "cpu",
                "--model",
                "tiny",
                "--steps",
                "1",
                "--warmup",
                "1",
                "--dir",
                d,
            ]
        )
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
        lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
        out = json.loads(lines[-1])
        assert out["n_gpus"] == 3
        assert out["ms_per_step"] > 0
