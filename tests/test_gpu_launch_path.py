"""GPU tests: the launch path of the gather and scatter kernels.

The launch tables travel through a ring of pinned slots (ops/hip/
table_ring.h), so a launch neither waits for the stream it enqueues on nor
holds the GIL. The oracle for bytes is torch's own ``contiguous().cpu()``
(and its CPU cast), for checksums the CPU psum64 of the same bytes - never
the code under test."""

import threading

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs a ROCm GPU", allow_module_level=True)

from torchsnapshot_amd import _csnap, integrity  # noqa: E402
from torchsnapshot_amd.ops import staging  # noqa: E402

_MB = 1024 * 1024


def _ref_bytes(t: torch.Tensor) -> bytes:
    c = t.detach().contiguous().cpu().reshape(-1)
    return bytes(c.view(torch.uint8).numpy()) if c.numel() else b""


@pytest.fixture
def small_pool(monkeypatch):
    """A private pool of 1 MiB pinned blocks: these tests hold many small
    batches at once and must not pin a 512 MiB block for each."""
    pool = staging.PinnedPool(block_size=_MB, block_count=64)
    monkeypatch.setattr(staging, "_pool", pool)
    return pool


def _engine() -> staging.StagingEngine:
    return staging.get_staging_engine(torch.device("cuda", 0))


def _pair(seed: int):
    """One contiguous and one transposed 64 KiB tensor, contents by seed."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randint(0, 256, (65536,), dtype=torch.uint8, device="cuda", generator=g)
    b = torch.randint(
        0, 256, (256, 256), dtype=torch.uint8, device="cuda", generator=g
    ).t()
    assert not b.is_contiguous()
    return [a, b]


def test_launch_does_not_wait_for_the_stream(small_pool):
    """A launch behind a queued 256 MiB gather returns while that gather is
    still running: at the link's <= 57 GB/s it needs at least 4.7 ms, a
    launch some tens of microseconds."""
    engine = _engine()
    big = [
        torch.randint(0, 256, (128 * _MB,), dtype=torch.uint8, device="cuda")
        for _ in range(2)
    ]
    small = [
        torch.randint(0, 256, (4096,), dtype=torch.uint8, device="cuda")
        for _ in range(2)
    ]
    # first launches load the code object; and leave a free pool block
    for _ in range(2):
        w = engine.stage(small)
        w.wait()
        w.release()
    torch.cuda.synchronize()

    # pinned allocations take a runtime-wide lock: the engine's background
    # pool warming, if still going, holds off for the two launches and
    # carries on afterwards
    with staging.pool_warming_paused():
        first = engine.stage(big)
        second = engine.stage(small)
        first_running = not _csnap.query(first._handle)
    first.wait()
    second.wait()
    try:
        assert first_running, (
            "the second stage() returned only after the 256 MiB gather "
            "queued before it had finished"
        )
        for batch, tensors in ((first, big), (second, small)):
            for i, t in enumerate(tensors):
                got = torch.frombuffer(batch.memoryview_of(i), dtype=torch.uint8)
                assert torch.equal(got, t.cpu()), i
    finally:
        first.release()
        second.release()


def test_ring_wrap_around():
    """More launches in flight than the ring has slots: the launch that
    wraps waits for the oldest slot, and no table is overwritten while a
    kernel still reads it."""
    n_batches = _csnap.table_ring_slots() + 5
    cur = torch.cuda.current_stream().cuda_stream
    batches = []
    per = 2 * 65536
    pinned = torch.zeros(n_batches * per, dtype=torch.uint8, pin_memory=True)
    for k in range(n_batches):
        tensors = _pair(1000 + k)
        items, offsets, total = staging.build_pack_items(tensors)
        assert total == per
        batches.append((tensors, offsets, staging._items_to_flat(items)))
    torch.cuda.synchronize()
    before = _csnap.pending_ops()
    handles = [
        _csnap.pack_d2h(
            flat, 2, 0, pinned.data_ptr() + k * per, per, cur, 0, 0
        )
        for k, (_, _, flat) in enumerate(batches)
    ]
    assert _csnap.pending_ops() == before + n_batches
    for h in handles:
        _csnap.wait(h)
    assert _csnap.pending_ops() == before
    host = bytes(pinned.numpy())
    for k, (tensors, offsets, _) in enumerate(batches):
        for t, off in zip(tensors, offsets):
            lo = k * per + off
            assert host[lo : lo + 65536] == _ref_bytes(t), (k, off)


def test_oversized_table_takes_the_fallback(small_pool):
    """More descriptors than a slot holds: the launch goes round the ring
    and every byte still arrives."""
    n = _csnap.table_ring_slot_bytes() // 100 + 8
    g = torch.Generator(device="cuda").manual_seed(7)
    src = torch.randint(0, 256, (n, 16), dtype=torch.uint8, device="cuda", generator=g)
    tensors = [src[i] for i in range(n)]
    batch = _engine().stage(tensors)
    batch.wait()
    want = src.cpu()
    for i in range(n):
        assert bytes(batch.memoryview_of(i)) == bytes(want[i].numpy()), i
    batch.release()
    # and the ring still works afterwards
    again = _engine().stage(tensors[:2])
    again.wait()
    assert bytes(again.memoryview_of(1)) == bytes(want[1].numpy())
    again.release()


def _scatter_round_trip(engine, seed: int) -> None:
    """Payload bytes in pinned memory -> one contiguous and one transposed
    device target through StagingEngine.scatter (the H2D ring)."""
    g = torch.Generator().manual_seed(seed)
    payload = torch.randint(0, 256, (2 * 65536,), dtype=torch.uint8, generator=g)
    block = staging.PinnedBlock(
        torch.empty(2 * 65536, dtype=torch.uint8, pin_memory=True), pooled=False
    )
    block.tensor.copy_(payload)
    a = torch.zeros(65536, dtype=torch.uint8, device="cuda")
    b = torch.zeros(256, 256, dtype=torch.uint8, device="cuda").t()
    engine.scatter(
        block, 2 * 65536, [(a, torch.uint8, 0), (b, torch.uint8, 65536)]
    )
    assert torch.equal(a.cpu(), payload[:65536])
    assert torch.equal(b.cpu().contiguous().reshape(-1), payload[65536:])


def test_concurrent_launchers(small_pool):
    """Eight staging threads and two restoring ones launch at once, none of
    them holding the GIL inside the extension: every byte is right and no
    op handle is left behind."""
    engine = _engine()
    warm = engine.stage(_pair(1))
    warm.wait()
    warm.release()
    torch.cuda.synchronize()
    before = _csnap.pending_ops()
    for round_no in range(2):
        errors = []
        start = threading.Barrier(10)

        def stager(tid):
            try:
                torch.cuda.set_device(0)
                start.wait()
                for k in range(8):
                    tensors = _pair(100 * tid + k + 10000 * round_no)
                    batch = engine.stage(tensors)
                    batch.wait()
                    for i, t in enumerate(tensors):
                        assert bytes(batch.memoryview_of(i)) == _ref_bytes(t), (
                            tid, k, i,
                        )
                    batch.release()
            except BaseException as e:  # noqa: BLE001 - reported below
                errors.append(e)

        def restorer(tid):
            try:
                torch.cuda.set_device(0)
                start.wait()
                for k in range(8):
                    _scatter_round_trip(engine, 77 * tid + k)
            except BaseException as e:  # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=stager, args=(i,)) for i in range(8)]
        threads += [threading.Thread(target=restorer, args=(i,)) for i in range(2)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        assert _csnap.pending_ops() == before


def test_cast_and_hash_through_the_ring(small_pool):
    """save_dtype narrowing and checksums in one batch: stored bytes equal
    torch's CPU cast, checksums the CPU psum64 of those bytes."""
    torch.manual_seed(1)
    tensors = [
        torch.randn(257, 129, device="cuda"),                  # cast
        torch.randn(257, 129, device="cuda"),                  # uncast fp32
        torch.arange(1000, device="cuda", dtype=torch.int64),  # int64
        torch.randn(1000, device="cuda").to(torch.bfloat16),   # bf16 source
        torch.randn(64, 96, device="cuda").t(),                # cast, transposed
        torch.empty(0, device="cuda"),                         # empty
        torch.randn(40, 1100, device="cuda")[:, :1030],        # cast, wide rows
        torch.randn(17, device="cuda"),                        # 34 stored bytes
    ]
    outs = [
        torch.bfloat16, None, None, None, torch.float16, torch.float16,
        torch.float16, torch.bfloat16,
    ]
    batch = _engine().stage(tensors, compute_checksums=True, out_dtypes=outs)
    batch.wait()
    assert batch.checksums is not None
    for i, (t, o) in enumerate(zip(tensors, outs)):
        stored = t.detach().cpu().contiguous()
        if o is not None and t.dtype == torch.float32:
            stored = stored.to(o)
        want = _ref_bytes(stored)
        assert bytes(batch.memoryview_of(i)) == want, i
        off = batch.offsets[i]
        assert off % 8 == 0
        digest = integrity.psum64_hexdigest(want, word_base=off // 8)
        got = "psum64:" + format(batch.checksums[i] % (1 << 64), "016x")
        assert got == digest, i
    total = sum(batch.checksums) % (1 << 64)
    whole = integrity.psum64_hexdigest(batch.slab_memoryview())
    assert "psum64:" + format(total, "016x") == whole
    batch.release()
