"""GPU tests: device restore through the scatter kernel.

One launch per read, straight out of pinned host memory, with bf16/f16 ->
f32 widening and the psum64 check fused in. The oracle throughout is
torch's CPU conversion of the same stored values (``.to(float32)``) and the
CPU psum64 of the same bytes — never the code under test."""

import asyncio
import glob
import os
from concurrent.futures import ThreadPoolExecutor

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from torchsnapshot_amd import Snapshot, StateDict, _csnap, integrity  # noqa: E402
from torchsnapshot_amd.io_preparers.sharded_tensor import (  # noqa: E402
    plan_shard_reads,
)
from torchsnapshot_amd.io_types import StageContext  # noqa: E402
from torchsnapshot_amd.manifest import Shard, TensorEntry  # noqa: E402
from torchsnapshot_amd.ops import staging  # noqa: E402
from torchsnapshot_amd.serialization import dtype_to_str  # noqa: E402
from torchsnapshot_amd.test_utils import tmp_snapshot_path  # noqa: E402

_STORED = [torch.bfloat16, torch.float16]
_STORED_IDS = ["bf16", "f16"]
_ALIGN = 256


def _bytes_of(t: torch.Tensor) -> bytes:
    c = t.detach().cpu().contiguous().reshape(-1)
    return bytes(c.view(torch.uint8).numpy()) if c.numel() else b""


def _unpack(targets, stored_dtypes, payloads, slab=False, word_base=None):
    """Lay the payloads out in one pinned buffer (256 B aligned each) and
    run ONE unpack_h2d over all of them. Returns (vecs, offsets, hashes);
    hashes is None unless ``word_base`` is given."""
    offsets, off = [], 0
    for p in payloads:
        offsets.append(off)
        off += (len(p) + _ALIGN - 1) // _ALIGN * _ALIGN
    total = max(off, 1)
    pinned = torch.zeros(total, dtype=torch.uint8, pin_memory=True)
    for p, o in zip(payloads, offsets):
        pinned[o : o + len(p)] = torch.frombuffer(bytearray(p), dtype=torch.uint8)
    items = staging.build_scatter_items(
        targets, stored_dtypes, offsets, flat_base=pinned.data_ptr()
    )
    dev_slab = (
        torch.empty(total, dtype=torch.uint8, device="cuda") if slab else None
    )
    hash_t = (
        torch.zeros(len(items), dtype=torch.uint64, device="cuda")
        if word_base is not None
        else None
    )
    torch.cuda.synchronize()
    handle = _csnap.unpack_h2d(
        staging._items_to_flat(items),
        len(items),
        dev_slab.data_ptr() if slab else 0,
        pinned.data_ptr(),
        total,
        torch.cuda.current_stream().cuda_stream,
        0,
        hash_t.data_ptr() if hash_t is not None else 0,
        word_base * 8 if word_base is not None else 0,
    )
    _csnap.wait(handle)
    hashes = (
        [int(v) % (1 << 64) for v in hash_t.cpu().tolist()]
        if hash_t is not None
        else None
    )
    return [it.vec for it in items], offsets, hashes


# ---------------------------------------------------------------------------
# 1. exhaustive widening, bit for bit
# ---------------------------------------------------------------------------

_N = 65536


def _all_patterns(stored: torch.dtype) -> torch.Tensor:
    return torch.arange(_N, dtype=torch.int32).to(torch.int16).view(stored)


def _misaligned_target() -> torch.Tensor:
    t = torch.zeros(_N + 1, device="cuda")[1:]
    assert t.data_ptr() % 8 == 4
    return t


# (name, make f32 target, expected vec, expected kind)
_WIDEN_LAYOUTS = [
    ("contiguous", lambda: torch.zeros(256, 256, device="cuda"), 16, "contig"),
    ("transposed", lambda: torch.zeros(256, 256, device="cuda").t(), 2, "narrow"),
    # 2731 * 24 = 65544 elements: the first 65536 hold the patterns
    ("narrow-rows", lambda: torch.zeros(2731, 32, device="cuda")[:, :24], 16, "narrow"),
    ("wide-rows", lambda: torch.zeros(32, 4096, device="cuda")[:, :2048], 16, "wide"),
    ("misaligned-base", _misaligned_target, 2, "contig"),
]


@pytest.fixture(scope="module")
def widen_oracle():
    """stored dtype -> (patterns, torch's CPU .to(float32) of them)."""
    out = {}
    for stored in _STORED:
        pat = _all_patterns(stored)
        out[stored] = (pat, pat.to(torch.float32))
    # bf16 -> f32 is the bit pattern shifted up, for every pattern
    pat, want = out[torch.bfloat16]
    shifted = (pat.view(torch.int16).to(torch.int32) & 0xFFFF) << 16
    assert torch.equal(want.view(torch.int32), shifted)
    return out


@pytest.mark.parametrize("slab", [False, True], ids=["direct", "slab"])
@pytest.mark.parametrize("stored", _STORED, ids=_STORED_IDS)
@pytest.mark.parametrize(
    "name,make,vec,kind", _WIDEN_LAYOUTS, ids=[c[0] for c in _WIDEN_LAYOUTS]
)
def test_exhaustive_widen(name, make, vec, kind, stored, slab, widen_oracle):
    pat, want = widen_oracle[stored]
    target = make()
    pad = target.numel() - _N
    assert 0 <= pad < 64
    payload = _bytes_of(pat) + b"\0" * (2 * pad)
    vecs, _, _ = _unpack([target], [stored], [payload], slab=slab)
    assert vecs == [vec]
    it = staging.build_scatter_items([target], [stored], [0])[0]
    got_kind = (
        "contig" if not it.outer_sizes
        else "wide" if it.row_bytes >= 2048 else "narrow"
    )
    assert got_kind == kind
    got = target.cpu().contiguous().reshape(-1)
    assert torch.count_nonzero(got[_N:]).item() == 0
    got = got[:_N]
    gb, wb = got.view(torch.int32), want.view(torch.int32)
    nan = torch.isnan(want)
    mism = (gb != wb) & ~nan
    assert not mism.any(), (
        int(mism.sum()),
        [hex(v & 0xFFFF) for v in pat.view(torch.int16)[mism][:8].tolist()],
    )
    assert torch.isnan(got[nan]).all()
    assert torch.equal(torch.signbit(got[nan]), torch.signbit(want[nan]))
    if stored == torch.bfloat16:
        assert torch.equal(gb, wb)  # NaN payloads included


# ---------------------------------------------------------------------------
# 2. work-unit edges
# ---------------------------------------------------------------------------


def _edge_targets(dtype):
    return [
        # 3 x 64 KiB + 2 stored bytes, contiguous
        ("3wu+2", lambda: torch.zeros(3 * 32768 + 1, dtype=dtype, device="cuda")),
        # 48-byte stored rows straddle the 64 KiB work-unit boundaries
        ("rows-4099x24", lambda: torch.zeros(4099, 32, dtype=dtype, device="cuda")[:, :24]),
    ]


@pytest.mark.parametrize("slab", [False, True], ids=["direct", "slab"])
@pytest.mark.parametrize(
    "stored,target_dtype",
    [
        (torch.bfloat16, torch.float32),
        (torch.float16, torch.float32),
        (torch.bfloat16, torch.bfloat16),
    ],
    ids=["bf16-widen", "f16-widen", "bf16-plain"],
)
@pytest.mark.parametrize("which", [0, 1], ids=["3wu+2", "rows-4099x24"])
def test_work_unit_edges(which, stored, target_dtype, slab):
    torch.manual_seed(3)
    _, make = _edge_targets(target_dtype)[which]
    target = make()
    src = torch.randn(tuple(target.shape)).to(stored)
    _unpack([target], [stored], [_bytes_of(src)], slab=slab)
    assert torch.equal(target.cpu(), src.to(target_dtype))


# ---------------------------------------------------------------------------
# 3. fused hash
# ---------------------------------------------------------------------------


def _hash_members():
    torch.manual_seed(4)
    # (target, stored dtype)
    return [
        (torch.zeros(300, 40, device="cuda"), torch.bfloat16),          # vec 16
        (torch.zeros(100, 8, device="cuda")[:, :3], torch.float32),     # vec 4
        (torch.zeros(33, 17, device="cuda").t(), torch.float16),        # vec 2
        (torch.zeros(70000, dtype=torch.bfloat16, device="cuda"), torch.bfloat16),
        (torch.zeros(13, dtype=torch.uint8, device="cuda"), torch.uint8),  # tail
    ]


@pytest.mark.parametrize("slab", [False, True], ids=["direct", "slab"])
def test_fused_hash_matches_cpu_psum64(slab):
    members = _hash_members()
    srcs = []
    for t, stored in members:
        if stored == torch.uint8:
            srcs.append(torch.randint(0, 256, tuple(t.shape), dtype=torch.uint8))
        else:
            srcs.append(torch.randn(tuple(t.shape)).to(stored))
    payloads = [_bytes_of(s) for s in srcs]
    word_base = 12345
    targets = [m[0] for m in members]
    stored = [m[1] for m in members]
    vecs, offsets, hashes = _unpack(
        targets, stored, payloads, slab=slab, word_base=word_base
    )
    assert {16, 4, 2} <= set(vecs)
    for i, (p, off) in enumerate(zip(payloads, offsets)):
        want = integrity.psum64_hexdigest(p, word_base=word_base + off // 8)
        assert "psum64:" + format(hashes[i], "016x") == want, f"member {i}"
    for t, s in zip(targets, srcs):
        assert torch.equal(t.cpu(), s.to(t.dtype))
    # one flipped byte changes that member's value, and only that one
    flipped = bytearray(payloads[2])
    flipped[5] ^= 0x10
    payloads2 = list(payloads)
    payloads2[2] = bytes(flipped)
    _, _, hashes2 = _unpack(
        targets, stored, payloads2, slab=slab, word_base=word_base
    )
    assert hashes2[2] != hashes[2]
    assert hashes2[:2] + hashes2[3:] == hashes[:2] + hashes[3:]


def test_unpack_refuses_bad_descriptors():
    """Refused on the host, before anything is launched."""
    dst = torch.zeros(64, 32, device="cuda")
    pinned = torch.zeros(8192, dtype=torch.uint8, pin_memory=True)
    stream = torch.cuda.current_stream().cuda_stream

    def call(items, total=8192, base=None, byte0=0):
        return _csnap.unpack_h2d(
            staging._items_to_flat(items), len(items), 0,
            pinned.data_ptr() if base is None else base, total, stream, 0,
            0, byte0,
        )

    narrowing, _, _ = staging.build_pack_items([dst], [torch.bfloat16])
    with pytest.raises(Exception, match="narrowing"):
        call(narrowing)
    widen = staging.build_scatter_items([dst], [torch.bfloat16], [0])
    with pytest.raises(Exception, match="outside the payload"):
        call(widen, total=4095)
    with pytest.raises(Exception, match="flat address"):
        call(widen, base=pinned.data_ptr() + 2)
    with pytest.raises(Exception, match="hash_byte0"):
        call(widen, byte0=4)
    # the other entry points keep refusing the widening codes
    with pytest.raises(Exception, match="cast"):
        _csnap.scatter_h2d(
            staging._items_to_flat(widen), 1, 0, pinned.data_ptr(), 8192,
            stream, 0,
        )
    with pytest.raises(Exception, match="scatter-only"):
        _csnap.pack_d2h(
            staging._items_to_flat(widen), 1, 0, pinned.data_ptr(), 8192,
            stream, 0,
        )
    torch.cuda.synchronize()
    assert torch.count_nonzero(dst).item() == 0


# ---------------------------------------------------------------------------
# 4. end to end
# ---------------------------------------------------------------------------


@pytest.fixture(params=["direct", "slab"])
def kernel_mode(request, monkeypatch):
    """The two TSAMD_RESTORE_MODE values that restore through the kernel."""
    monkeypatch.setenv("TSAMD_RESTORE_MODE", request.param)
    return request.param


def _count_scatter_calls(monkeypatch):
    calls = []
    orig = staging.StagingEngine.scatter

    def wrapped(self, pinned_block, nbytes, members, *args, **kwargs):
        calls.append(len(members))
        return orig(self, pinned_block, nbytes, members, *args, **kwargs)

    monkeypatch.setattr(staging.StagingEngine, "scatter", wrapped)
    return calls


@pytest.mark.parametrize("stored", _STORED, ids=_STORED_IDS)
@pytest.mark.parametrize("chunked", [False, True], ids=["whole", "chunked"])
def test_save_dtype_restores_into_f32(
    stored, chunked, toggle_batching, kernel_mode, monkeypatch
):
    if chunked:
        monkeypatch.setenv("TSAMD_MAX_CHUNK_SIZE_BYTES", "1024")
    torch.manual_seed(5)
    src = StateDict(
        w=torch.randn(300, 130, device="cuda"),
        wt=torch.randn(64, 96, device="cuda"),
        s=torch.tensor(2.5, device="cuda"),
        b=torch.randn(77, device="cuda"),
    )
    calls = _count_scatter_calls(monkeypatch)
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": src}, save_dtype=stored)
        out = StateDict(
            w=torch.zeros(300, 130, device="cuda"),
            wt=torch.zeros(96, 64, device="cuda").t(),  # transposed target
            s=torch.tensor(0.0, device="cuda"),
            b=torch.zeros(77, device="cuda"),
        )
        assert not out["wt"].is_contiguous()
        snap.restore({"sd": out})
    # A dim-0 chunk of the transposed target is a non-dense view, for which
    # torch cannot rule out internal overlap: scatter_plan declines it, and
    # with batching on that one member takes its whole span to the torch
    # path. Every other combination must reach the kernel.
    batching_off = toggle_batching
    if not chunked or batching_off:
        assert calls, "the restore did not go through the scatter kernel"
    for k in ("w", "wt", "s", "b"):
        want = src[k].cpu().to(stored).to(torch.float32)
        assert out[k].dtype == torch.float32
        assert torch.equal(out[k].cpu(), want), k


@pytest.mark.parametrize(
    "dtype",
    [torch.float8_e4m3fn, torch.uint8, torch.bfloat16],
    ids=["fp8", "u8", "bf16"],
)
def test_same_dtype_restore(dtype, toggle_batching, kernel_mode, monkeypatch):
    torch.manual_seed(6)

    def rnd(*shape):
        # every byte value occurs; built on the host, moved as bytes
        u8 = torch.randint(0, 256, shape, dtype=torch.uint8)
        return u8.view(dtype).cuda() if dtype.itemsize == 1 else (
            torch.randn(*shape).to(dtype).cuda()
        )

    def zeros(*shape):
        return torch.zeros(shape, dtype=torch.uint8).view(dtype).cuda() if (
            dtype.itemsize == 1
        ) else torch.zeros(shape, dtype=dtype, device="cuda")

    src = StateDict(a=rnd(129, 33), b=rnd(1000), c=rnd(7, 5))
    calls = _count_scatter_calls(monkeypatch)
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": src})
        out = StateDict(a=zeros(129, 33), b=zeros(1000), c=zeros(5, 7).t())
        snap.restore({"sd": out})
    assert calls
    for k in ("a", "b", "c"):
        assert torch.equal(
            out[k].cpu().contiguous().view(torch.uint8),
            src[k].cpu().contiguous().view(torch.uint8),
        ), k


# ---------------------------------------------------------------------------
# 5. one launch per span
# ---------------------------------------------------------------------------


def test_one_launch_per_span(kernel_mode, monkeypatch):
    from torchsnapshot_amd import batcher

    torch.manual_seed(7)
    src = StateDict(
        **{f"t{i}": torch.randn(50 + i, 3, device="cuda") for i in range(40)}
    )

    def zeros():
        return StateDict(
            **{f"t{i}": torch.zeros(50 + i, 3, device="cuda") for i in range(40)}
        )

    spans = []
    orig_consume = batcher.BatchedBufferConsumer.consume_buffer

    async def counted(self, ctx, buf):
        spans.append(len(self.members))
        return await orig_consume(self, ctx, buf)

    monkeypatch.setattr(batcher.BatchedBufferConsumer, "consume_buffer", counted)
    calls = _count_scatter_calls(monkeypatch)
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": src})
        out = zeros()
        snap.restore({"sd": out})
        assert spans and sum(spans) == 40
        assert len(calls) == len(spans)
        assert sorted(calls) == sorted(spans)

        del calls[:]
        monkeypatch.setenv("TSAMD_RESTORE_MODE", "torch")
        out_torch = zeros()
        snap.restore({"sd": out_torch})
        assert calls == []
    for k in src:
        assert torch.equal(out[k], src[k]), k
        assert torch.equal(out_torch[k], out[k]), k


# ---------------------------------------------------------------------------
# 6. no transient HBM
# ---------------------------------------------------------------------------


def test_direct_restore_allocates_no_payload_copy(monkeypatch):
    """The .to(device) path allocates at least the 32 MiB stored buffer
    (plus the converting copy's source); the kernel reads pinned memory."""
    monkeypatch.setenv("TSAMD_RESTORE_MODE", "direct")
    torch.manual_seed(8)
    t = torch.randn(16 * 1024 * 1024, device="cuda")  # 64 MiB fp32
    fp32_bytes = t.numel() * 4
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": StateDict(w=t)}, save_dtype=torch.bfloat16)
        out = StateDict(w=torch.zeros_like(t))
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        snap.restore({"sd": out})
        rise = torch.cuda.max_memory_allocated() - before
    print("max_memory_allocated rise:", rise)
    assert rise < fp32_bytes // 4, rise
    assert torch.equal(out["w"], t.to(torch.bfloat16).to(torch.float32))
    del t, out
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# 7. verified restore
# ---------------------------------------------------------------------------


def test_verified_restore_and_corruption(toggle_batching, kernel_mode, monkeypatch):
    monkeypatch.setenv("TSAMD_CHECKSUM", "1")
    monkeypatch.setenv("TSAMD_SLAB_SIZE_THRESHOLD_BYTES", str(1024 * 1024))
    torch.manual_seed(9)
    src = StateDict(
        big=torch.randn(1024, 1024, device="cuda"),  # 2 MiB stored: own file
        s0=torch.randn(199, 33, device="cuda"),
        s1=torch.randn(64, 64, device="cuda"),
        s2=torch.randn(5, device="cuda"),
    )

    def zeros():
        return StateDict(
            big=torch.zeros(1024, 1024, device="cuda"),
            s0=torch.zeros(199, 33, device="cuda"),
            s1=torch.zeros(64, 64, device="cuda").t(),
            s2=torch.zeros(5, device="cuda"),
        )

    calls = _count_scatter_calls(monkeypatch)
    with tmp_snapshot_path() as path:
        snap = Snapshot.take(path, {"sd": src}, save_dtype=torch.bfloat16)
        monkeypatch.setenv("TSAMD_VERIFY_CHECKSUM", "1")
        out = zeros()
        snap.restore({"sd": out})
        assert calls
        for k in src:
            want = src[k].cpu().to(torch.bfloat16).to(torch.float32)
            assert torch.equal(out[k].cpu(), want), k

        payloads = [
            p
            for p in glob.glob(os.path.join(path, "**"), recursive=True)
            if os.path.isfile(p)
            and not p.endswith((".snapshot_metadata", ".checksums"))
        ]
        for target in payloads:  # the big tensor's file, then the small ones
            pos = min(64, os.path.getsize(target) - 1)
            with open(target, "r+b") as f:
                f.seek(pos)
                b = f.read(1)
                f.seek(pos)
                f.write(bytes([b[0] ^ 0x40]))
            with pytest.raises(RuntimeError, match="checksum mismatch"):
                snap.restore({"sd": zeros()})
            with open(target, "r+b") as f:
                f.seek(pos)
                f.write(b)
        snap.restore({"sd": zeros()})  # repaired: clean again


# ---------------------------------------------------------------------------
# 8. shards
# ---------------------------------------------------------------------------


def _feed(read_reqs, payload_of):
    """Drive the consumers the way the read pipeline does: the storage
    layer fills the buffer buf_alloc hands out, then consume_buffer runs."""

    async def run():
        with ThreadPoolExecutor(max_workers=2) as ex:
            ctx = StageContext(executor=ex)
            for req in read_reqs:
                data = payload_of[req.path]
                assert req.buf_alloc is not None
                buf = req.buf_alloc(len(data))
                buf[:] = data
                try:
                    await req.consumer.consume_buffer(ctx, buf)
                finally:
                    req.consumer.close()

    asyncio.run(run())


@pytest.mark.parametrize("stored", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("split", ["rows", "cols"])
def test_reshard_2_to_3(split, stored, kernel_mode, monkeypatch):
    torch.manual_seed(10)
    rows, cols = 90, 66
    full = torch.randn(rows, cols).to(stored)
    dim = 0 if split == "rows" else 1
    n = full.shape[dim]
    shards, payload_of = [], {}
    for i, (off, ln) in enumerate([(0, n // 2), (n // 2, n - n // 2)]):
        piece = full.narrow(dim, off, ln)
        offsets = [0, 0]
        offsets[dim] = off
        entry = TensorEntry(
            location=f"shard{i}",
            serializer="buffer",
            dtype=dtype_to_str(stored),
            shape=list(piece.shape),
        )
        shards.append(Shard(offsets=offsets, sizes=list(piece.shape), tensor=entry))
        payload_of[entry.location] = _bytes_of(piece)
    out = torch.zeros(rows, cols, device="cuda")  # f32: bf16 shards widen
    targets = []
    for off, ln in [(0, n // 3), (n // 3, n // 3), (2 * (n // 3), n - 2 * (n // 3))]:
        offsets = [0, 0]
        offsets[dim] = off
        targets.append((out.narrow(dim, off, ln), offsets))
    calls = _count_scatter_calls(monkeypatch)
    reqs = plan_shard_reads(shards, targets)
    assert len(reqs) == 2
    _feed(reqs, payload_of)
    if split == "rows":
        # every overlap is a contiguous run of its stored shard
        assert len(calls) == len(reqs) and sum(calls) == 4
    else:
        assert calls == []  # N-d sub-boxes keep the torch path
    assert torch.equal(out.cpu(), full.to(torch.float32))
