"""staging.pool_warming_paused(): background pool warming holds off for the
duration and then warms what it had left. Runs on a pool whose blocks are
plain host memory, so no GPU is needed."""

import threading

import torch

from torchsnapshot_amd.ops import staging


class _PlainPool(staging.PinnedPool):
    def __init__(self, gate: threading.Event, started: threading.Event) -> None:
        super().__init__(block_size=1024, block_count=8)
        self._gate = gate
        self._started = started

    def _alloc(self, nbytes: int) -> torch.Tensor:
        self._started.set()
        assert self._gate.wait(30)
        return torch.empty(nbytes, dtype=torch.uint8)


def test_pause_stops_warming_and_resumes_the_rest(monkeypatch):
    monkeypatch.setattr(staging, "_warm_thread", None)
    monkeypatch.setattr(staging, "_warm_left", [None, 0])
    gate, started = threading.Event(), threading.Event()
    pool = _PlainPool(gate, started)
    staging._start_warming(pool, 4 * 1024, background=True)
    first = staging._warm_thread
    assert started.wait(30)  # the thread is inside its first allocation
    gate.set()
    with staging.pool_warming_paused():
        assert not first.is_alive()
        held = pool._allocated
        assert 1 <= held <= 4
        assert staging._warm_left[1] == (4 - held) * 1024
    resumed = staging._warm_thread
    if held < 4:
        assert resumed is not first
        resumed.join(30)
    assert pool._allocated == 4
    assert staging._warm_left[1] == 0


def test_pause_without_a_warming_thread_is_a_no_op(monkeypatch):
    monkeypatch.setattr(staging, "_warm_thread", None)
    monkeypatch.setattr(staging, "_warm_left", [None, 0])
    with staging.pool_warming_paused():
        pass
    assert staging._warm_thread is None
