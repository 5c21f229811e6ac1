"""GPU test: one mixed batch through the routine that the scan and the
fingerprint share. It guards the two places that routine can go wrong: the
fold of several descriptors' results into their tensor's, and the merge of
the fallback's answers for the tensors the builders declined."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from torchsnapshot_amd.ops import staging  # noqa: E402

DEV = torch.device("cuda", 0)
NAN, INF = float("nan"), float("inf")


class _CountingExt:
    """staging._csnap with every call through it recorded by name."""

    def __init__(self, real):
        self._real = real
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def counted(*args, **kwargs):
            self.calls.append(name)
            return fn(*args, **kwargs)

        return counted


def test_mixed_batch_one_call_each(monkeypatch):
    engine = staging.get_staging_engine(DEV)
    assert engine._use_ext
    torch.manual_seed(0)
    vector = torch.randn(3 * 16384 + 5, device=DEV)
    vector[1] = NAN
    vector[-1] = INF
    # 4 outer dims after collapsing: strided, through the kernels
    strided = torch.zeros(4, 4, 4, 4, 4, 4, 4, 4, device=DEV)[
        :, :2, :, :2, :, :2, :, :2
    ]
    strided[1, 1, 2, 0, 3, 1, 0, 1] = NAN
    # 7 outer dims after collapsing: one more than the kernels take
    declined = torch.zeros(4, 4, 4, 4, 4, 4, 4, 4, device=DEV)[
        :2, :2, :2, :2, :2, :2, :2, :2
    ]
    declined[1, 0, 1, 1, 0, 1, 0, 1] = NAN
    declined[0, 1, 0, 0, 1, 0, 1, 0] = -INF
    split = torch.randn(5, 8192, device=DEV)  # 3 pieces of at most 64 KiB
    split[0, 0] = NAN
    split[2, 8191] = INF
    split[4, 17] = NAN
    tensors = [
        torch.empty(0, device=DEV),
        vector,
        strided,
        declined,
        torch.arange(1000, dtype=torch.int64, device=DEV),
        split,
        vector,
    ]
    cpu = [t.cpu() for t in tensors]

    monkeypatch.setattr(staging, "_KERNEL_MAX_BYTES", 65536)
    items, classes = staging.build_scan_items(tensors)
    assert [None if its is None else len(its) for its in items] == [
        0, 4, 1, None, None, 3, 4,
    ]
    assert classes[3] == staging.SCAN_F32 and classes[4] is None
    pieces = staging.build_fingerprint_items(tensors, split_bytes=65536)
    assert [None if its is None else len(its) for its in pieces] == [
        0, 4, 1, None, 1, 3, 4,
    ]

    ext = _CountingExt(staging._csnap)
    monkeypatch.setattr(staging, "_csnap", ext)
    counts = engine.scan_nonfinite(tensors)
    assert ext.calls == ["scan_nonfinite"]
    want_counts = [staging.torch_count_nonfinite(t) for t in cpu]
    print(counts, want_counts)
    assert want_counts == [(0, 0), (1, 1), (1, 0), (1, 1), (0, 0), (2, 1), (1, 1)]
    for i, (got, want) in enumerate(zip(counts, want_counts)):
        assert got == want, i

    sums = engine.fingerprint(tensors, split_bytes=65536)
    assert ext.calls == ["scan_nonfinite", "fingerprint_tensors"]
    want_sums = [staging.host_fingerprint(t) for t in cpu]
    print(sums, want_sums)
    for i, (got, want) in enumerate(zip(sums, want_sums)):
        assert got == want, i
    assert sums[0] == 0 and sums[1] == sums[6] != 0
