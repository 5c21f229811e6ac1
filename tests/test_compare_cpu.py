"""Snapshot.compare without a GPU: the torch expression and the merge
against hand-written cases, the host path end to end, the CLI, and
DescKind::Compare of ops/hip/desc_check.h in a stand-alone program built
with ASan + UBSan (nothing is loaded into Python under a sanitizer)."""

import itertools
import math
import os
import shutil
import subprocess

import pytest
import torch

from torchsnapshot_amd import Snapshot, StateDict, TensorDiff
from torchsnapshot_amd.__main__ import main
from torchsnapshot_amd.compare import CompareSink
from torchsnapshot_amd.ops.staging import merge_diff, torch_tensor_diff

NAN, INF = math.nan, math.inf
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "desc_check_compare_selftest.cpp")
INCLUDE = os.path.join(REPO, "torchsnapshot_amd", "ops", "hip")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.parametrize(
    "stored, live, want",
    [
        ([1.0, 2.0, 3.0], [1.0, 2.5, 1.0], [3, 2, 0, 2.0, 4.25, 14.0]),
        ([0.0, 1.0], [-0.0, 1.0], [2, 1, 0, 0.0, 0.0, 1.0]),
        ([NAN, INF, INF, 2.0], [NAN, INF, 1.0, NAN], [4, 2, 2, 0.0, 0.0, 0.0]),
        ([], [], [0, 0, 0, 0.0, 0.0, 0.0]),
    ],
)
def test_torch_tensor_diff_floats(stored, live, want):
    assert torch_tensor_diff(torch.tensor(stored), torch.tensor(live)) == want


def test_torch_tensor_diff_bits_and_dtypes():
    a = torch.tensor([NAN, 1.0])
    b = a.clone()
    b.view(torch.int32)[0] ^= 1  # another NaN payload
    assert torch_tensor_diff(a, b) == [2, 1, 1, 0.0, 0.0, 1.0]
    # bf16 stored against f32 live: widened exactly, then compared
    v = torch.tensor([1.0, 1.0 + 2.0**-10])
    assert torch_tensor_diff(v.to(torch.bfloat16), v) == [2, 1, 0, 2.0**-10, 2.0**-20, 2.0]
    ints = torch_tensor_diff(torch.tensor([1, 2, 3]), torch.tensor([1, 5, 3]))
    assert ints == [3, 1, 0, None, None, None]
    z = torch.tensor([1 + 2j, 3 + 4j])
    assert torch_tensor_diff(z, torch.tensor([1 + 2j, 3 - 4j]))[:2] == [2, 1]


def test_merge_diff_and_piece_order():
    a, b = [3, 1, 0, 0.5, 0.1, 1e16], [2, 2, 1, 2.0, 0.2, 1.0]
    assert merge_diff(a, b) == [5, 3, 1, 2.0, 0.1 + 0.2, 1e16 + 1.0]
    assert merge_diff([1, 0, 0, None, None, None], [2, 1, 0, None, None, None])[3:] == [None] * 3
    # 2^53 + 1 + 1 depends on the order: 2^53 + 2 only when the ones add first.
    # Pieces merge by key, here ones first, whatever order they arrive in
    terms = {((0,), 0): 1.0, ((0,), 8): 1.0, ((4,), 0): 2.0**53}
    assert (2.0**53 + 1.0) + 1.0 != (1.0 + 1.0) + 2.0**53
    for order in itertools.permutations(terms):
        sink = CompareSink()
        for key in order:
            sink.add("p", key, [1, 0, 0, 0.0, terms[key], terms[key]])
        got = sink.result()["p"]
        assert got.sum_sq == got.ref_sum_sq == 2.0**53 + 2.0 and got.n == 3


@pytest.fixture
def two_states(tmp_path):
    torch.manual_seed(0)
    a = StateDict(w=torch.randn(40, 30), b=torch.randn(7), idx=torch.arange(9), gone=torch.ones(2),
                  z=torch.tensor(1.5), kind=torch.ones(2), step=1)
    Snapshot.take(str(tmp_path / "a"), {"m": a})
    b = StateDict(w=a["w"].clone(), b=a["b"].clone(), idx=a["idx"].clone(),
                  new=torch.zeros(3), z=torch.ones(3), kind="text", step=2)
    b["w"][3, 4] += 0.5
    b["b"][2] *= 3
    b["idx"] = torch.arange(10)
    return tmp_path, a, b


def test_snapshot_compare_on_host(two_states):
    tmp_path, a, b = two_states
    kept = {k: v.clone() for k, v in b.items() if isinstance(v, torch.Tensor)}
    found = Snapshot(str(tmp_path / "a")).compare({"m": b})
    assert set(found) == {"m/w", "m/b", "m/idx", "m/new", "m/gone", "m/z", "m/kind"}
    assert found["m/z"].note == "shape () vs (3,)"  # a stored 0-d tensor
    assert found["m/kind"].note == "not a tensor in app_state"
    assert found["m/new"].note == "missing in snapshot" and found["m/new"].n == 0
    assert found["m/gone"].note == "missing in app_state"
    assert found["m/idx"].note == "shape (9,) vs (10,)"
    w = found["m/w"]
    assert (w.n, w.n_diff, w.n_nonfinite_diff) == (1200, 1, 0)
    assert w.max_abs == (b["w"].double() - a["w"].double()).abs().max().item()
    assert (w.rms_err, w.rel_err) == (math.sqrt(w.sum_sq / 1200), math.sqrt(w.sum_sq / w.ref_sum_sq))
    assert TensorDiff(n=4, sum_sq=0.0, ref_sum_sq=0.0).rel_err is None and not w.equal
    assert w.ref_sum_sq == pytest.approx((a["w"].double() ** 2).sum().item(), rel=1e-12)
    assert all(torch.equal(b[k], v) for k, v in kept.items())
    assert all(d.equal for d in Snapshot(str(tmp_path / "a")).compare({"m": a}).values())


def test_cli_orders_by_relative_error(two_states, capsys):
    tmp_path, _, b = two_states
    Snapshot.take(str(tmp_path / "b"), {"m": b})
    assert main(["compare", str(tmp_path / "b"), str(tmp_path / "a")]) == 1
    lines = capsys.readouterr().out.strip().splitlines()
    assert [ln.split(":")[0] for ln in lines[:2]] == ["m/b", "m/w"]
    assert {ln.split(":")[0] for ln in lines[2:]} == {"m/idx", "m/new", "m/gone", "m/z", "m/kind"}
    assert main(["compare", str(tmp_path / "a"), str(tmp_path / "a")]) == 0


def test_desc_check_compare_under_asan_ubsan(tmp_path):
    names = (os.environ.get("CXX"), "g++", "clang++", "c++")
    cxx = next((shutil.which(n) for n in names if n and shutil.which(n)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "selftest")
    build = subprocess.run([cxx, *FLAGS, f"-I{INCLUDE}", SRC, "-o", exe], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "selftest OK" in run.stdout, run.stdout + run.stderr
