"""GPU tests: replicated_check= on device state, world 2 on one shared
device (gloo), through the fingerprint kernel."""

import os
import tempfile

import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from torchsnapshot_amd import ReplicatedStateMismatchError, Snapshot, StateDict  # noqa: E402
from torchsnapshot_amd.test_utils import run_multiprocess_gpu  # noqa: E402


def _mismatch_is_refused(tmpdir: str, is_async: bool) -> None:
    rank = dist.get_rank()
    path = os.path.join(tmpdir, "snap")
    torch.manual_seed(0)  # the same state on both ranks
    sd = StateDict(
        t=torch.randn(300, 130, device="cuda").t(),
        h=torch.randn(70001, device="cuda"),
    )
    kw = dict(replicated=["**"], save_dtype={"**/h": torch.float16})
    Snapshot.take(path, {"sd": sd}, replicated_check="error", **kw)
    want = {k: v.clone() for k, v in sd.items()}
    if rank == 1:
        sd["t"][129, 299] += 1
        sd["h"][70000] = 7.0  # survives the float16 rounding
    take = Snapshot.async_take if is_async else Snapshot.take
    with pytest.raises(ReplicatedStateMismatchError) as ei:
        take(path, {"sd": sd}, replicated_check="error", **kw)  # both ranks
    report = ei.value.report
    assert sorted(report) == ["sd/h", "sd/t"]
    assert all(len(set(v)) == 2 for v in report.values())
    out = StateDict(**{k: torch.zeros_like(v) for k, v in want.items()})
    Snapshot(path).restore({"sd": out})  # the earlier commit is intact
    assert torch.equal(out["t"], want["t"])
    assert torch.equal(out["h"], want["h"].to(torch.float16).float())


@pytest.mark.parametrize("is_async", [False, True], ids=["take", "async_take"])
def test_mismatch_is_refused_world2_shared_gpu(is_async):
    with tempfile.TemporaryDirectory() as d:
        run_multiprocess_gpu(
            2, _mismatch_is_refused, d, is_async, backend="gloo", share_device=True
        )
