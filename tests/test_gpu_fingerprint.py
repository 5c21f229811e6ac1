"""GPU tests: the fingerprint kernel against the host psum64, exactly."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from torchsnapshot_amd import integrity  # noqa: E402
from torchsnapshot_amd.ops import staging  # noqa: E402

DEV = torch.device("cuda", 0)
WU = 64 * 1024
U8, F32, BF16, F16 = torch.uint8, torch.float32, torch.bfloat16, torch.float16

ENGINE = staging.get_staging_engine(DEV)
assert ENGINE._use_ext  # the values below come from the kernel


def _ref(t, stored=None):
    c = t.detach().cpu()
    c = (c if stored is None else c.to(stored)).contiguous()
    return integrity.psum64_value(c.reshape(-1).view(U8).numpy())


def _rand(shape, dtype):  # random bytes viewed as dtype
    n = torch.Size(shape).numel() * dtype.itemsize
    g = torch.Generator().manual_seed(n)
    raw = torch.randint(0, 256, (n,), dtype=U8, generator=g).to(DEV)
    return raw.view(dtype).reshape(shape)


def _layouts(dtype):
    if dtype == U8:
        sizes = (1, 7, 8, 9, 4099, WU, WU + 1, 3 * WU + 2)
        return [_rand((n,), U8) for n in sizes] + [_rand((4100,), U8)[1:]]
    if dtype == F32:
        expanded = torch.zeros(1, 16, device=DEV).expand(8, 16)
        expanded._base.copy_(_rand((1, 16), F32))
        return [
            _rand((40, 1024), F32)[:, :520],  # 2080 B rows, vec 16
            _rand((5, 1024), F32)[:, 1:514],  # vec 4
            _rand((4099, 32), F32)[:, :24],
            _rand((129, 33), F32).t(),
            expanded,
            _rand((6, 5, 4, 33), F32).permute(3, 1, 0, 2),
        ]
    if dtype == BF16:
        return [_rand((4099, 32), BF16)[:, :24]]
    if dtype == torch.complex128:
        return [_rand((33, 17), dtype).t()]  # one-element rows at vec 16
    return [_rand((1001,), dtype)]


@pytest.mark.parametrize("dtype", [U8, F32, BF16, torch.complex128, torch.float64])
def test_plain_layouts(dtype):
    tensors = _layouts(dtype)
    tensors = tensors[:1] + [torch.empty(0, dtype=dtype, device=DEV)] + tensors[1:]
    bases = [t if t._base is None else t._base for t in tensors]
    before = [b.clone() for b in bases]
    got = ENGINE.fingerprint(tensors)
    assert got == [_ref(t) for t in tensors] and got[1] == 0
    for b, snap in zip(bases, before):  # read-only
        assert torch.equal(b.view(U8), snap.view(U8))


_SPECIALS = [
    0.0, -0.0, 1e-40, -1e-45, 1e-6, -6e-8, 65504.0, 65519.99, 65520.0,
    -65520.0, 3.4028234e38, float("inf"), -float("inf"), 1.0, -2.5, 1e-3,
]
_NAN_BITS = [0x7F800001, 0xFFC12345 - 2**32, 0x7FFFFFFF, 0x7F80FFFF]


@pytest.mark.parametrize("nans", [False, True], ids=["finite", "nans"])
@pytest.mark.parametrize("stored", [BF16, F16], ids=str)
def test_cast_descriptors(stored, nans):
    torch.manual_seed(0)
    vals = torch.cat([torch.tensor(_SPECIALS), torch.randn(47) * 300])
    if nans:
        vals = torch.cat([vals, torch.tensor(_NAN_BITS, dtype=torch.int32).view(F32)])
    tensors = [
        torch.zeros(70001, device=DEV),
        torch.zeros(40, 1024, device=DEV)[:, :520],
        torch.zeros(129, 33, device=DEV).t(),
        torch.zeros(4099, 32, device=DEV)[:, :24],
    ]
    for t in tensors:
        t.copy_(vals.repeat(t.numel() // len(vals) + 1)[: t.numel()].reshape(t.shape))
    got = ENGINE.fingerprint(tensors, [stored] * 4)
    if nans:
        # the contract: the hash of what the gather would store
        batch = ENGINE.stage(tensors, out_dtypes=[stored] * 4)
        batch.wait()
        want = [integrity.psum64_value(batch.memoryview_of(i)) for i in range(4)]
        batch.release()
    else:
        want = [_ref(t, stored) for t in tensors]
    assert got == want


def test_stride_independence():
    x = _rand((129, 33), F32)
    y = x.t().contiguous().t()
    a, b = ENGINE.fingerprint([x, y])
    assert x.stride() != y.stride() and a == b == _ref(x)


@pytest.mark.parametrize("pos", [0, 3 * WU + 1, WU])
def test_one_bit_changes_the_fingerprint(pos):
    t = _rand((3 * WU + 2,), U8).clone()
    (before,) = ENGINE.fingerprint([t])
    t[pos] ^= 1
    (after,) = ENGINE.fingerprint([t])
    assert before != after and after == _ref(t)


def test_split_declined_and_disabled(monkeypatch):
    tensors = [
        _rand((300, 520), F32)[:, :500],
        _rand((999, 331), U8),  # an odd piece offset: vec drops to 1
        (_rand((900, 130), torch.int16) / 7.0).t(),  # finite float32
        _rand([2] * 8, F32).permute(*range(7, -1, -1)),  # 8 outer dims
    ]
    stored = [None, None, BF16, None]
    want = [_ref(t, s) for t, s in zip(tensors, stored)]
    items = staging.build_fingerprint_items(tensors, stored, split_bytes=3 * WU)
    assert [its and len(its) > 1 for its in items] == [True, True, True, None]
    assert ENGINE.fingerprint(tensors, stored, split_bytes=3 * WU) == want
    assert ENGINE.fingerprint(tensors, stored) == want
    monkeypatch.setenv("TSAMD_DISABLE_HIP_STAGING", "1")
    disabled = staging.StagingEngine(DEV)
    monkeypatch.setattr(staging._csnap, "fingerprint_tensors", None)
    assert not disabled._use_ext and disabled.fingerprint(tensors, stored) == want


# a widening cast code, a negative stride, a flat_off that splits a word
@pytest.mark.parametrize(
    "index,value,match",
    [(18, 3, "widening"), (12, 2**64 - 4096, "not aligned"), (1, 8, "flat_off")],
)
def test_extension_refuses(index, value, match):
    t = torch.zeros(40, 1024, device=DEV)[:, :520]
    flat = staging._items_to_flat(staging.build_fingerprint_items([t])[0])
    stream = torch.cuda.current_stream().cuda_stream
    assert staging._csnap.fingerprint_tensors(flat, 1, stream, 0) == [0]
    flat[index] = value
    with pytest.raises(RuntimeError, match="fingerprint_tensors: .*" + match):
        staging._csnap.fingerprint_tensors(flat, 1, stream, 0)
