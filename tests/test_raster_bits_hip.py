"""The rasteriser's bits, pinned: every digest and integer of tests/golden/raster_bits.json (made by tests/golden/make_raster_bits.py
from the commit the file records) is recomputed with the tree under test and compared for equality.  No tolerance: an edit that
keeps the arithmetic keeps every bit of every image, radius, final_T, n_contrib and gradient, every instance and group count, and
every value of the three *_workspace_bytes functions."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_raster_bits", os.path.join(GOLDEN, "make_raster_bits.py"))
bits = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(bits)

with open(os.path.join(GOLDEN, "raster_bits.json")) as _f:
    PINNED = json.load(_f)


def differences(tag, got, want):
    if isinstance(want, dict) and isinstance(got, dict):
        return [d for k in sorted(set(want) | set(got)) for d in differences(f"{tag}: {k}", got.get(k), want.get(k))]
    return [] if got == want else [f"{tag}: {got!r}, pinned {want!r}"]


def test_the_fixture_covers_every_case():
    assert set(PINNED["cases"]) == set(bits.CASES) and PINNED["commit"] and PINNED["rocm"] and PINNED["device"]


@pytest.mark.parametrize("name", sorted(bits.CASES))
def test_bits_are_those_of_the_pinned_commit(hip_device, name):
    diff = differences(name, bits.CASES[name](hip_device), PINNED["cases"][name])
    assert not diff, f"bits differ from commit {PINNED['commit']} ({PINNED['rocm']}, {PINNED['device']}):\n" + "\n".join(diff)
