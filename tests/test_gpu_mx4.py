"""Block-scaled fp4 on the device: the bytes the gather kernel stores and the
tensors the scatter kernel restores against the float64 reference of
docs/format.md, at tolerance 0."""

import pytest
import torch

from torchsnapshot_amd import Snapshot, StateDict, integrity
from torchsnapshot_amd.ops import staging

from _mx4_reference import assert_error_bound, edge_values4, mx4_reference
from _mx_reference import decoded_as, edge_values, mx_reference

pytestmark = pytest.mark.gpu

MX4 = "mxfp4_e2m1"
SAME = dict(rtol=0, atol=0, equal_nan=True)


def _layout(case, base):
    """The case's view of a base tensor, and the class its descriptor takes."""
    if case == "aligned_view":  # rows of 64 = 2 x 32 elements
        return base.reshape(40, 128)[:, :64], 8
    if case == "general_view":  # rows of 24: blocks cross rows at odd nibbles
        return base.reshape(37, 50)[:, :24], 1
    if case == "transposed":  # rows of one element
        return base.reshape(65, 33).t(), 1
    return base, 8  # contiguous, `case` elements


_BASE_NUMEL = {"aligned_view": 40 * 128, "general_view": 37 * 50, "transposed": 65 * 33}


@pytest.mark.parametrize("checksum", [False, True], ids=["plain", "hashed"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize(
    "case", [1, 31, 32, 33, 131072 + 37, "aligned_view", "general_view", "transposed"]
)
def test_kernels_match_reference(case, dtype, checksum):
    dev = torch.device("cuda", 0)
    base = edge_values4(_BASE_NUMEL.get(case, case), dtype)
    src, vec = _layout(case, base.to(dev))
    payload, decoded, E = mx4_reference(src.cpu())
    assert_error_bound(src.cpu(), decoded, E)
    assert payload.numel() == 17 * (-(-src.numel() // 32))
    assert staging.build_pack_items([src], [MX4])[0][0].vec == vec

    engine = staging.get_staging_engine(dev)
    batch = engine.stage([src], compute_checksums=checksum, out_dtypes=[MX4])
    batch.wait()
    try:
        stored = torch.frombuffer(bytearray(batch.memoryview_of(0)), dtype=torch.uint8)
        assert torch.equal(stored, payload)
        psum = integrity.psum64_value(payload.numpy())
        if checksum:
            assert batch.checksums == [psum]
        # the scatter kernel, out of the block the gather filled
        out, _ = _layout(case, torch.zeros_like(base, device=dev))
        expected = (psum, 0) if checksum else None
        engine.scatter(batch.pinned, payload.numel(), [(out, MX4, 0)], expected)
    finally:
        batch.release()
    want = decoded_as(decoded, dtype).reshape(out.shape)
    torch.testing.assert_close(out.cpu(), want, **SAME)


@pytest.mark.parametrize("checksum", ["0", "1"])
def test_mixed_slab_take_restore(tmp_path, monkeypatch, checksum):
    """One slab with mxfp4 members of both dtypes and both classes, an mxfp8
    member, a bf16-cast member and plain members; the restore is verified on
    the device."""
    monkeypatch.setenv("TSAMD_CHECKSUM", checksum)
    monkeypatch.setenv("TSAMD_VERIFY_CHECKSUM", checksum)
    dev = torch.device("cuda", 0)
    host = dict(
        mx4_a=edge_values4(700, torch.float32).reshape(7, 100),
        mx4_b=edge_values4(2048 + 5, torch.bfloat16),
        mx4_t=edge_values4(33 * 65, torch.float32).reshape(65, 33).t(),
        mx4_v=edge_values4(40 * 128, torch.bfloat16).reshape(40, 128)[:, :64],
        mx8=edge_values(300, torch.float32),
        cast=torch.randn(300),
        keep=torch.randn(129, dtype=torch.float16),
        ints=torch.arange(77),
    )
    src = StateDict(**{k: v.to(dev) for k, v in host.items()})
    rule = {"**/mx4_*": MX4, "**/mx8": "mxfp8_e4m3", "**/cast": torch.bfloat16}
    snap = Snapshot.take(str(tmp_path / "s"), {"m": src}, save_dtype=rule)
    manifest = snap.get_manifest()
    assert len({manifest[f"0/m/{k}"]["location"] for k in host}) == 1
    lo, hi = manifest["0/m/mx4_b"]["byte_range"]
    assert hi - lo == 17 * 65  # 2053 elements: 65 blocks
    out = StateDict(**{k: torch.zeros_like(v) for k, v in src.items()})
    snap.restore({"m": out})
    for k, v in host.items():
        if k.startswith("mx"):
            ref = mx4_reference if k.startswith("mx4") else mx_reference
            want = decoded_as(ref(v)[1], v.dtype).reshape(v.shape)
            torch.testing.assert_close(out[k].cpu(), want, **SAME)
    assert torch.equal(out["cast"].cpu(), host["cast"].bfloat16().float())
    assert torch.equal(out["keep"].cpu(), host["keep"])
    assert torch.equal(out["ints"].cpu(), host["ints"])
