"""GPU tests: the gather kernel's fused f32 -> bf16/f16 cast.

The oracle throughout is torch's CPU cast of the same values,
``t.cpu().contiguous().to(dst)`` — never the code under test."""

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from torchsnapshot_amd import Snapshot, StateDict, integrity  # noqa: E402
from torchsnapshot_amd.ops import staging  # noqa: E402
from torchsnapshot_amd.test_utils import tmp_snapshot_path  # noqa: E402

_TARGETS = [torch.bfloat16, torch.float16]
_TARGET_IDS = ["bf16", "f16"]
_MODES = ["direct", "slab"]


def _oracle(t: torch.Tensor, dst: torch.dtype) -> torch.Tensor:
    return t.detach().cpu().contiguous().to(dst)


def _oracle_bytes(t: torch.Tensor, dst: torch.dtype) -> bytes:
    o = _oracle(t, dst).reshape(-1)
    if o.numel() == 0:
        return b""
    return bytes(o.view(torch.uint8).numpy())


def _ref_bytes(t: torch.Tensor) -> bytes:
    """Uncast reference serialization: plain torch contiguous + cpu."""
    c = t.detach().contiguous().cpu().reshape(-1)
    if c.numel() == 0:
        return b""
    return bytes(c.view(torch.uint8).numpy())


def _stage_one(t: torch.Tensor, dst: torch.dtype) -> bytes:
    engine = staging.get_staging_engine(t.device)
    batch = engine.stage([t], out_dtypes=[dst])
    batch.wait()
    got = bytes(batch.memoryview_of(0))
    batch.release()
    return got


# ---------------------------------------------------------------------------
# numerics, bit-exact
# ---------------------------------------------------------------------------

_LOW_HALVES = [
    0x0000, 0x0001, 0x0FFF, 0x1000, 0x1001, 0x2FFF,
    0x3000, 0x3001, 0x7FFF, 0x8000, 0x8001, 0xFFFF,
]


def _from_bits(bits: torch.Tensor) -> torch.Tensor:
    """int64 tensor of u32 bit patterns -> fp32 tensor."""
    signed = torch.where(bits >= 2**31, bits - 2**32, bits)
    return signed.to(torch.int32).view(torch.float32)


def _input_set_a() -> torch.Tensor:
    hi = torch.arange(65536, dtype=torch.int64).unsqueeze(1) << 16
    lo = torch.tensor(_LOW_HALVES, dtype=torch.int64).unsqueeze(0)
    return _from_bits((hi | lo).reshape(-1))


def _input_set_b() -> torch.Tensor:
    """For every finite f16 value h: h, the exact midpoint between h and its
    successor (next larger magnitude; 65536 past the largest finite), and
    the fp32 neighbours of that midpoint."""
    h = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    h = h[torch.isfinite(h)]
    mag = h.abs().to(torch.float64)
    nxt_bits = (h.abs().view(torch.int16).to(torch.int32) + 1).to(torch.int16)
    nxt = nxt_bits.view(torch.float16).to(torch.float64)
    nxt = torch.where(torch.isinf(nxt), torch.tensor(65536.0, dtype=torch.float64), nxt)
    sign = torch.where(
        h.view(torch.int16) < 0,
        torch.tensor(-1.0, dtype=torch.float64),
        torch.tensor(1.0, dtype=torch.float64),
    )
    mid64 = sign * (mag + nxt) / 2
    mid = mid64.to(torch.float32)
    # midpoints of adjacent f16 values need 12 significant bits: exact in fp32
    assert torch.equal(mid.to(torch.float64), mid64)
    mid_bits = mid.view(torch.int32)
    return torch.cat(
        [
            h.to(torch.float32),
            mid,
            (mid_bits - 1).view(torch.float32),
            (mid_bits + 1).view(torch.float32),
        ]
    )


def _check_bits(x_cpu: torch.Tensor, dst: torch.dtype, nan_cap: float) -> float:
    got_b = _stage_one(x_cpu.cuda(), dst)
    got = torch.frombuffer(bytearray(got_b), dtype=torch.int16)
    want = x_cpu.to(dst)
    assert got.numel() == want.numel()
    nan_in = torch.isnan(x_cpu)
    share = nan_in.double().mean().item()
    # the NaN exemption is capped; everything else is compared bit for bit
    assert share <= nan_cap, share
    mism = (got != want.view(torch.int16)) & ~nan_in
    assert not mism.any(), (
        int(mism.sum()),
        [hex(v & 0xFFFFFFFF) for v in x_cpu.view(torch.int32)[mism][:8].tolist()],
    )
    assert torch.isnan(got.view(dst)[nan_in]).all()
    return share


@pytest.mark.parametrize("dst", _TARGETS, ids=_TARGET_IDS)
def test_numerics_set_a_bit_exact(dst):
    x = _input_set_a()
    assert x.numel() == 786432
    share = _check_bits(x, dst, nan_cap=0.005)
    # 2 signs x 128 NaN high halves x 12 low halves, minus the two infs
    assert share == pytest.approx(3070 / 786432)


def test_numerics_set_b_f16_bit_exact():
    x = _input_set_b()
    share = _check_bits(x, torch.float16, nan_cap=0.005)
    assert share == 0.0


# ---------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------


def _misaligned_base() -> torch.Tensor:
    t = torch.randn(70001, device="cuda").view(-1)[1:]
    assert t.data_ptr() % 8 == 4
    return t


_LAYOUTS = [
    ("contiguous", lambda: torch.randn(257, 129, device="cuda")),
    ("wide-strided", lambda: torch.randn(40, 1100, device="cuda")[:, :1030]),
    ("transposed", lambda: torch.randn(512, 512, device="cuda").t()),
    ("narrow", lambda: torch.randn(1000, 64, device="cuda")[100:900]),
    ("three-elem-rows", lambda: torch.randn(700, 8, device="cuda")[:, :3]),
    ("permuted-3d", lambda: torch.randn(33, 5, 7, device="cuda").permute(2, 0, 1)),
    ("misaligned-base", _misaligned_base),
    # 8-byte stores (narrow rows) and 16-byte stores (wide rows)
    ("four-elem-rows", lambda: torch.randn(300, 12, device="cuda")[:, :4]),
    ("wide-vec16", lambda: torch.randn(40, 2048, device="cuda")[:, :1024]),
    ("scalar", lambda: torch.tensor(3.14159, device="cuda")),
    ("empty", lambda: torch.empty(0, 4, device="cuda")),
]


@pytest.mark.parametrize("mode", _MODES)
@pytest.mark.parametrize("dst", _TARGETS, ids=_TARGET_IDS)
@pytest.mark.parametrize("name,make", _LAYOUTS, ids=[c[0] for c in _LAYOUTS])
def test_cast_layouts(name, make, dst, mode, monkeypatch):
    monkeypatch.setenv("TSAMD_STAGE_MODE", mode)
    torch.manual_seed(0)
    t = make()
    assert _stage_one(t, dst) == _oracle_bytes(t, dst)


def test_layout_cases_hit_every_strategy():
    """The layout list covers contiguous, wide-row and narrow-row
    addressing and every vector width."""
    from torchsnapshot_amd.ops.staging import build_pack_items

    seen = set()
    for _name, make in _LAYOUTS:
        t = make()
        it = build_pack_items([t], [torch.bfloat16])[0][0]
        if it.nbytes == 0:
            continue
        if not it.outer_sizes:
            kind = "contig"
        elif it.row_bytes >= 2048:
            kind = "wide"
        else:
            kind = "narrow"
        seen.add((kind, it.vec))
    assert {k for k, _ in seen} == {"contig", "wide", "narrow"}
    assert {v for _, v in seen} == {16, 8, 4, 2}
    assert ("wide", 16) in seen and ("wide", 4) in seen
    assert ("narrow", 8) in seen and ("narrow", 2) in seen


# ---------------------------------------------------------------------------
# mixed batch, checksums
# ---------------------------------------------------------------------------


def _mixed():
    torch.manual_seed(1)
    tensors = [
        torch.randn(257, 129, device="cuda"),                 # cast
        torch.randn(257, 129, device="cuda"),                 # uncast fp32
        torch.arange(1000, device="cuda", dtype=torch.int64), # int64
        torch.randn(1000, device="cuda").to(torch.bfloat16),  # bf16 source
        torch.randn(64, 96, device="cuda").t(),               # cast, transposed
        torch.empty(0, device="cuda"),                        # empty
        torch.randn(40, 1100, device="cuda")[:, :1030],       # cast, wide rows
    ]
    outs = [
        torch.bfloat16, None, None, None, torch.float16, torch.float16,
        torch.float16,
    ]
    return tensors, outs


@pytest.mark.parametrize("mode", _MODES)
def test_mixed_batch_one_stage_call(mode, monkeypatch):
    monkeypatch.setenv("TSAMD_STAGE_MODE", mode)
    tensors, outs = _mixed()
    engine = staging.get_staging_engine(tensors[0].device)
    batch = engine.stage(tensors, out_dtypes=outs)
    batch.wait()
    for i, (t, o) in enumerate(zip(tensors, outs)):
        got = bytes(batch.memoryview_of(i))
        if o is not None and t.dtype == torch.float32:
            assert got == _oracle_bytes(t, o), f"tensor {i}"
        else:
            assert got == _ref_bytes(t), f"tensor {i}"
    batch.release()


@pytest.mark.parametrize("mode", _MODES)
def test_cast_checksums_cover_stored_bytes(mode, monkeypatch):
    monkeypatch.setenv("TSAMD_STAGE_MODE", mode)
    tensors, outs = _mixed()
    tensors.append(torch.randn(17, device="cuda"))  # 34 stored bytes: tail
    outs.append(torch.bfloat16)
    engine = staging.get_staging_engine(tensors[0].device)
    batch = engine.stage(tensors, compute_checksums=True, out_dtypes=outs)
    batch.wait()
    assert batch.checksums is not None
    total = sum(batch.checksums) % (1 << 64)
    want = integrity.psum64_hexdigest(batch.slab_memoryview())
    assert "psum64:" + format(total, "016x") == want
    for i, off in enumerate(batch.offsets):
        assert off % 8 == 0
        member = integrity.psum64_hexdigest(
            bytes(batch.memoryview_of(i)), word_base=off // 8
        )
        got = "psum64:" + format(batch.checksums[i] % (1 << 64), "016x")
        assert got == member, f"tensor {i}"
    batch.release()


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------


def _e2e_state():
    torch.manual_seed(2)
    return StateDict(
        big=torch.randn(1024, 1024, device="cuda"),  # 2 MiB stored: own file
        s0=torch.randn(199, 33, device="cuda"),
        s1=torch.randn(64, 64, device="cuda").t(),
        s2=torch.randn(5, device="cuda"),
        idx=torch.arange(77, device="cuda"),
        step=3,
    )


def _e2e_zeros():
    return StateDict(
        big=torch.zeros(1024, 1024, device="cuda"),
        s0=torch.zeros(199, 33, device="cuda"),
        s1=torch.zeros(64, 64, device="cuda"),
        s2=torch.zeros(5, device="cuda"),
        idx=torch.zeros(77, dtype=torch.int64, device="cuda"),
        step=0,
    )


@pytest.mark.parametrize("dst", _TARGETS, ids=_TARGET_IDS)
@pytest.mark.parametrize("use_async", [False, True], ids=["take", "async_take"])
def test_snapshot_save_dtype_round_trip(use_async, dst, monkeypatch):
    monkeypatch.setenv("TSAMD_CHECKSUM", "1")
    monkeypatch.setenv("TSAMD_SLAB_SIZE_THRESHOLD_BYTES", str(1024 * 1024))
    sd = _e2e_state()
    saved = {
        k: (v.clone() if isinstance(v, torch.Tensor) else v)
        for k, v in sd.items()
    }
    with tmp_snapshot_path() as path:
        if use_async:
            pending = Snapshot.async_take(path, {"sd": sd}, save_dtype=dst)
            for v in sd.values():
                if isinstance(v, torch.Tensor):
                    v.zero_()
            snap = pending.wait()
        else:
            snap = Snapshot.take(path, {"sd": sd}, save_dtype=dst)
        man = snap.get_manifest()
        assert not man["0/sd/big"]["location"].startswith("batched/")
        assert man["0/sd/s0"]["location"].startswith("batched/")
        from torchsnapshot_amd.serialization import dtype_to_str

        for k in ("big", "s0", "s1", "s2"):
            assert man[f"0/sd/{k}"]["dtype"] == dtype_to_str(dst)
        assert man["0/sd/idx"]["dtype"] == dtype_to_str(torch.int64)

        monkeypatch.setenv("TSAMD_VERIFY_CHECKSUM", "1")
        out = _e2e_zeros()
        snap.restore({"sd": out})
        for k in ("big", "s0", "s1", "s2"):
            want = saved[k].cpu().contiguous().to(dst).to(torch.float32)
            assert out[k].dtype == torch.float32
            assert torch.equal(out[k].cpu(), want), k
        assert torch.equal(out["idx"], saved["idx"])
        assert out["step"] == 3


def test_sync_take_makes_no_device_staging_copy(monkeypatch):
    """save_dtype narrows inside the gather: no second device copy of the
    state. (Casting in the prepare hook allocates half the fp32 size.)"""
    monkeypatch.setenv("TSAMD_STAGE_MODE", "direct")
    t = torch.randn(16 * 1024 * 1024, device="cuda")  # 64 MiB fp32
    fp32_bytes = t.numel() * 4
    sd = StateDict(w=t)
    with tmp_snapshot_path() as path:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        snap = Snapshot.take(path, {"sd": sd}, save_dtype=torch.bfloat16)
        rise = torch.cuda.max_memory_allocated() - before
        assert rise < fp32_bytes // 4, rise
        got = snap.read_object("0/sd/w")
        assert torch.equal(got, _oracle(t, torch.bfloat16))
    del t, sd
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# rejection
# ---------------------------------------------------------------------------


def test_scatter_rejects_cast_descriptor():
    from torchsnapshot_amd import _csnap
    from torchsnapshot_amd.ops.staging import _items_to_flat, build_pack_items

    dst = torch.zeros(64, 32, device="cuda")
    items, _, total = build_pack_items([dst], [torch.bfloat16])
    pinned = torch.zeros(total, dtype=torch.uint8, pin_memory=True)
    with pytest.raises(Exception, match="cast"):
        _csnap.scatter_h2d(
            _items_to_flat(items), len(items), 0, pinned.data_ptr(), total,
            torch.cuda.current_stream().cuda_stream, 0,
        )
    torch.cuda.synchronize()
    assert torch.count_nonzero(dst).item() == 0


def test_unsupported_pair_raises_on_device():
    t = torch.zeros(8, dtype=torch.float64, device="cuda")
    engine = staging.get_staging_engine(t.device)
    with pytest.raises(ValueError):
        engine.stage([t], out_dtypes=[torch.bfloat16])
