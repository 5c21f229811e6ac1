"""The per-take planning memo of the DTensor preparer changes no manifest.

One take saves DTensors on two meshes (1-D and 2-D, gloo) with Shard and
Replicate placements that share shapes, so every memo key is hit more than
once and the two meshes must not be mistaken for each other. The same state
is then saved with the memo bypassed; the committed metadata files must be
equal byte for byte (a list object shared between entries would already
change how they serialise)."""

import contextlib
import os
import tempfile

import pytest
import torch
import torch.distributed as dist

from torchsnapshot_amd.test_utils import run_multiprocess

pytestmark = pytest.mark.timeout(300)


class _Holder:
    def __init__(self, sd):
        self.sd = sd

    def state_dict(self):
        return self.sd

    def load_state_dict(self, sd):
        self.sd = sd


def _state():
    from torch.distributed.device_mesh import init_device_mesh
    from torch.distributed.tensor import distribute_tensor
    from torch.distributed.tensor.placement_types import Replicate, Shard

    mesh1 = init_device_mesh("cpu", (4,))
    mesh2 = init_device_mesh("cpu", (2, 2))
    torch.manual_seed(11)
    a, b, c = torch.rand(48, 8), torch.rand(48, 8), torch.rand(7, 8)
    return {
        # same (mesh, placements, shape) twice: one layout, two entries
        "m1_s0_a": distribute_tensor(a, mesh1, [Shard(0)]),
        "m1_s0_b": distribute_tensor(b, mesh1, [Shard(0)]),
        # same mesh and shape, other placements
        "m1_s1": distribute_tensor(a, mesh1, [Shard(1)]),
        "m1_rep": distribute_tensor(a, mesh1, [Replicate()]),
        # same shape and placements class on the other mesh
        "m2_rep_s0": distribute_tensor(a, mesh2, [Replicate(), Shard(0)]),
        "m2_s0_rep": distribute_tensor(b, mesh2, [Shard(0), Replicate()]),
        "m2_s0_s1": distribute_tensor(a, mesh2, [Shard(0), Shard(1)]),
        "m2_rep_rep": distribute_tensor(b, mesh2, [Replicate(), Replicate()]),
        # uneven shards (7 rows over 4 and over 2 ranks), again on both
        "m1_uneven": distribute_tensor(c, mesh1, [Shard(0)]),
        "m2_uneven": distribute_tensor(c, mesh2, [Replicate(), Shard(0)]),
    }


def _save_both_ways(tmpdir: str) -> None:
    from torchsnapshot_amd import Snapshot, snapshot as snapshot_mod
    from torchsnapshot_amd.io_preparers import dtensor as dtensor_mod

    sd = _state()
    entered = []
    real = dtensor_mod.planning_memo

    @contextlib.contextmanager
    def counting():
        with real():
            yield
            memo = dtensor_mod._plan_state.memo
            entered.append(
                (len(memo.meshes), len(memo.replica_sets), len(memo.layouts))
            )

    snapshot_mod.planning_memo = counting
    Snapshot.take(os.path.join(tmpdir, "memo"), {"obj": _Holder(sd)})
    # 2 meshes; 3 + 4 distinct (mesh, placements); with the shapes, 4 + 5
    # distinct triples for the 10 tensors
    assert entered == [(2, 7, 9)], entered
    assert getattr(dtensor_mod._plan_state, "memo", None) is None

    snapshot_mod.planning_memo = contextlib.nullcontext
    Snapshot.take(os.path.join(tmpdir, "plain"), {"obj": _Holder(sd)})
    dist.barrier()


def test_manifest_equal_with_and_without_memo_world4():
    from torchsnapshot_amd import Snapshot
    from torchsnapshot_amd.manifest import METADATA_FILENAME

    with tempfile.TemporaryDirectory() as d:
        run_multiprocess(4, _save_both_ways, d)
        with open(os.path.join(d, "memo", METADATA_FILENAME), "rb") as f:
            memo = f.read()
        with open(os.path.join(d, "plain", METADATA_FILENAME), "rb") as f:
            plain = f.read()
        assert memo == plain
        man = Snapshot(os.path.join(d, "memo")).get_manifest()
        assert man["0/obj/m2_rep_s0"]["mesh"] == [[0, 1], [2, 3]]
        assert man["0/obj/m1_s0_a"]["mesh"] == [0, 1, 2, 3]
        out = Snapshot(os.path.join(d, "memo")).read_object("0/obj/m2_s0_s1")
        torch.manual_seed(11)
        assert torch.equal(out, torch.rand(48, 8))
