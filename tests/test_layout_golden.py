"""The three descriptor builders against recorded PackItems.

``tests/golden/pack_items.json`` holds, field for field, what
build_pack_items (plain and cast) and build_scan_items returned for every
layout case of the three CPU layout suites before the builders shared one
layout-to-rows helper. Addresses are stored relative to the tensor's
storage base, so they do not depend on where the allocator put it (torch
aligns CPU storage to 64 bytes, so ``vec`` does not either)."""

import json
import os

import pytest
import torch

from torchsnapshot_amd.ops import staging

from test_cast_layout import _FP32_CASES
from test_nonfinite_layout import _LAYOUT_CASES
from test_staging_layout import _CASES

GOLDEN = os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "golden", "pack_items.json"
)
_CAST_TARGETS = {"bf16": torch.bfloat16, "f16": torch.float16}


def _item_fields(it, t):
    return {
        "src_off": it.src_ptr - t.untyped_storage().data_ptr(),
        "flat_offset": it.flat_offset,
        "nbytes": it.nbytes,
        "row_bytes": it.row_bytes,
        "outer_sizes": list(it.outer_sizes),
        "outer_strides": list(it.outer_strides),
        "vec": it.vec,
        "cast": it.cast,
    }


def current_items():
    """What the builders return now, in the fixture's shape."""
    out = {"pack": {}, "cast": {}, "scan": {}}
    for name, make in _CASES:
        t = make()
        assert t.untyped_storage().data_ptr() % 16 == 0
        items, offsets, total = staging.build_pack_items([t])
        out["pack"][name] = {
            "item": _item_fields(items[0], t),
            "offsets": offsets,
            "total": total,
        }
    for name, make in _FP32_CASES:
        for key, dst in _CAST_TARGETS.items():
            t = make()
            assert t.untyped_storage().data_ptr() % 16 == 0
            items, offsets, total = staging.build_pack_items([t], [dst])
            out["cast"][f"{name}/{key}"] = {
                "item": _item_fields(items[0], t),
                "offsets": offsets,
                "total": total,
            }
    for name, make in _LAYOUT_CASES:
        t = make()
        assert t.untyped_storage().data_ptr() % 16 == 0
        (its,), (cls,) = staging.build_scan_items([t])
        out["scan"][name] = {
            "class": cls,
            "items": None if its is None else [_item_fields(i, t) for i in its],
        }
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def current():
    return current_items()


@pytest.mark.parametrize("builder", ["pack", "cast", "scan"])
def test_builders_match_recorded_items(builder, golden, current):
    want, got = golden[builder], current[builder]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], (builder, name)
