"""GPU tests: re-saving device state onto a committed path (payload files
overwritten in place)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from torchsnapshot_amd import Snapshot, StateDict  # noqa: E402
from torchsnapshot_amd.test_utils import tmp_snapshot_path  # noqa: E402

MIB = 1 << 20


def _state(seed: int) -> StateDict:
    g = torch.Generator(device="cuda").manual_seed(seed)

    def randn(*shape, dtype=torch.float32):
        return torch.randn(
            *shape, generator=g, device="cuda", dtype=torch.float32
        ).to(dtype)

    return StateDict(
        # three contiguous 1.5 MiB bf16 tensors (gather-pack slab)
        w0=randn(768, 1024, dtype=torch.bfloat16),
        w1=randn(768, 1024, dtype=torch.bfloat16),
        w2=randn(768, 1024, dtype=torch.bfloat16),
        # transposed 512x768 fp32 (strided gather)
        wt=randn(768, 512).t(),
        # 1 MiB + 14 B: just over the in-place threshold, odd length
        tail=randn((MIB + 14) // 2, dtype=torch.bfloat16),
    )


def _zeros_like_state(sd: StateDict) -> StateDict:
    return StateDict(
        **{k: torch.zeros_like(v, memory_format=torch.contiguous_format)
           for k, v in sd.items()}
    )


def _assert_restores(path: str, sd: StateDict) -> None:
    out = _zeros_like_state(sd)
    Snapshot(path).restore({"sd": out})
    for k, v in sd.items():
        assert out[k].shape == v.shape
        assert torch.equal(out[k].cpu(), v.cpu()), k


@pytest.mark.parametrize("checksums", [False, True], ids=["plain", "verified"])
def test_resave_device_state_bit_exact(monkeypatch, checksums):
    if checksums:
        monkeypatch.setenv("TSAMD_CHECKSUM", "1")
        monkeypatch.setenv("TSAMD_VERIFY_CHECKSUM", "1")
    first, second = _state(1), _state(2)
    assert not torch.equal(first["w0"], second["w0"])
    assert first["tail"].numel() * 2 == MIB + 14
    with tmp_snapshot_path() as path:
        Snapshot.take(path, {"sd": first})
        _assert_restores(path, first)
        Snapshot.take(path, {"sd": second})
        _assert_restores(path, second)

