"""CPU checks of pixie_amd/csrc/part_seg_math.h (compiled for the host by tests/host_harness/part_seg_math_host.cpp, g++
-ffp-contract=off): both stages of the part segmentation through the same lane shares, butterfly, epilogue, offset table and cube
bisection as the kernels of part_segmentation.hip, against the float64 restatement of tests/_part_seg_ref.py.

Bars.  Labels equal the float64 restatement wherever its top-two margin exceeds tau = 2 C 2^-24 (tests/test_part_seg_ref.py shows
that at most 1 % of a scene lies inside); counts equal a bincount of the labels; the material grid and the voted grid are EQUAL;
|score - float64 score| <= C 2^-24 / (2 T) + 8 2^-24 (derived in tests/_part_seg_ref.py).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _part_seg_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "part_seg_math_host.cpp")
FP, U8, I8, U16, I64 = (C.POINTER(t) for t in (C.c_float, C.c_uint8, C.c_int8, C.c_uint16, C.c_int64))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("pseg_host") / "libpart_seg_math_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_ps_offsets.argtypes = [I8]
    h.hh_ps_half.argtypes, h.hh_ps_half.restype = [C.c_uint16], C.c_float
    h.hh_ps_stage_a.argtypes = [C.c_int] * 5 + [U16, U8, FP, C.c_float, I8, FP, I64]
    h.hh_ps_vote.argtypes, h.hh_ps_vote.restype = [C.c_int] * 3 + [I8, C.c_int, I8], C.c_int64
    h.hh_ps_material.argtypes = [C.c_int64, I8, FP, C.c_int, C.c_float, FP]
    return h


def host_stage_a(h, sc, temperature=0.1):
    d, hh, w = sc["shape"]
    feat = np.ascontiguousarray(sc["features"]).view(np.uint16)
    mask = np.ascontiguousarray(sc["mask"], np.uint8)
    q = np.ascontiguousarray(sc["queries"], np.float32)
    labels, scores, counts = np.zeros((d, hh, w), np.int8), np.zeros((d, hh, w), np.float32), np.zeros(33, np.int64)
    rc = h.hh_ps_stage_a(d, hh, w, feat.shape[-1], q.shape[0], feat.ctypes.data_as(U16), mask.ctypes.data_as(U8), q.ctypes.data_as(FP),
                         temperature, labels.ctypes.data_as(I8), scores.ctypes.data_as(FP), counts.ctypes.data_as(I64))
    assert rc == 0
    return labels, scores, counts


def host_material(h, labels, props, background_id=7):
    out = np.zeros(labels.shape + (4,), np.float32)
    p = np.ascontiguousarray(props, np.float32)
    h.hh_ps_material(labels.size, np.ascontiguousarray(labels).ctypes.data_as(I8), p.ctypes.data_as(FP), len(p), background_id, out.ctypes.data_as(FP))
    return out


def host_vote(h, grid, k):
    voted = np.zeros(grid.shape, np.int8)
    g = np.ascontiguousarray(grid, np.int8)
    slow = h.hh_ps_vote(*grid.shape, g.ctypes.data_as(I8), k, voted.ctypes.data_as(I8))
    return voted, int(slow)


def compare_stage_a(sc, labels, scores, counts, ref, temperature=0.1):
    """shared with nothing: the GPU tests have their own copy of the same comparisons"""
    mask, channels, parts = sc["mask"], sc["features"].shape[-1], len(sc["queries"])
    assert np.all(labels[~mask] == -1) and np.all(np.isnan(scores[~mask]))
    got, got_scores = labels[mask].astype(np.int64), scores[mask].astype(np.float64)
    clear = ref["margin"] > R.tau(channels)
    assert np.array_equal(got[clear], ref["labels"][clear])
    assert got.min(initial=0) >= 0 and got.max(initial=0) < parts
    assert np.array_equal(counts[:parts], np.bincount(got, minlength=parts)) and counts[32] == mask.sum()
    fine = ~np.isnan(ref["scores"])
    assert np.array_equal(np.isnan(got_scores), ~fine)
    err = np.abs(got_scores[fine] - ref["scores"][fine])                  # every voxel, inside tau or not
    bar = R.score_bar(channels, temperature)
    print(f"{sc['name']}: {len(got)} voxels, {int((~clear).sum())} inside tau, worst |score - ref| {err.max() if len(err) else 0.0:.3e}, bar {bar:.3e}")
    assert np.all(err <= bar)


@pytest.mark.parametrize("name", list(R.STAGE_A))
def test_header_equals_the_restatement_stage_a(host, name):
    sc = R.stage_a_scene(name)
    ref = R.stage_a64(sc["features"], sc["mask"], sc["queries"])
    labels, scores, counts = host_stage_a(host, sc)
    compare_stage_a(sc, labels, scores, counts, ref)
    assert np.array_equal(host_material(host, labels, sc["props"]), R.material_fill(labels, sc["props"]))
    if name == "zero_row":
        assert labels[sc["mask"]][3] == 0 and np.isnan(scores[sc["mask"]][3])


def test_duplicate_query_rows_tie_to_the_lower_index(host):
    sc = R.duplicate_scene()
    labels, scores, counts = host_stage_a(host, sc)
    uniq = R.stage_a64(sc["features"], sc["mask"], sc["queries"][[0, 1, 3]])
    got = labels[sc["mask"]]
    assert not np.any(got == 2) and np.any(got == 1) and counts[2] == 0
    clear = uniq["margin"] > R.tau(128)
    assert np.array_equal(got[clear], np.array([0, 1, 3])[uniq["labels"]][clear])


def test_another_temperature(host):
    sc = R.stage_a_scene("c768k5")
    ref = R.stage_a64(sc["features"], sc["mask"], sc["queries"], temperature=0.5)
    compare_stage_a(sc, *host_stage_a(host, sc, temperature=0.5), ref, temperature=0.5)


def test_half_widening_is_exact_for_every_bit_pattern(host):
    bits = np.arange(65536, dtype=np.uint16)
    want = bits.view(np.float16).astype(np.float32)
    got = np.array([host.hh_ps_half(int(b)) for b in bits], np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got[~np.isnan(want)].view(np.uint32), want[~np.isnan(want)].view(np.uint32))


@pytest.mark.parametrize("name,parts,k,slow", [("ball", 2, 200, True), ("ball", 6, 10, False), ("ball", 6, 7, False), ("plate", 6, 200, True),
                                               ("plate", 2, 7, False), ("strays", 2, 200, True), ("strays", 6, 10, True)])
def test_header_vote_equals_the_restatement(host, name, parts, k, slow):
    grid = R.vote_scene(name, parts)
    voted, n_slow = host_vote(host, grid, k)
    ref = R.vote(grid, k)
    print(f"{name} K={parts} k={k}: {int((grid >= 0).sum())} voxels, slow path {n_slow}")
    assert np.array_equal(voted, ref["voted"])
    assert (n_slow > 0) == slow, "the scene is there to run (or not to run) the cube bisection"


def test_offset_table_is_every_offset_up_to_25_in_rule_order(host):
    buf = (C.c_int8 * (4 * 520))()
    n = host.hh_ps_offsets(buf)
    t = np.frombuffer(buf, np.int8).reshape(520, 4)[:n].astype(int)
    assert n == 515
    assert np.array_equal((t[:, :3] ** 2).sum(axis=1), t[:, 3]) and t[0].tolist() == [0, 0, 0, 0]
    # sorted by (n, C-order index of the neighbour) for any grid: the index is monotone in (di, dj, dk) taken lexicographically
    key = [(r[3], r[0], r[1], r[2]) for r in t.tolist()]
    assert key == sorted(key) and len(set(key)) == 515
    r = np.arange(-5, 6)
    assert n == int(((r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2) <= 25).sum())


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of pixie_part_seg_desc as gcc lays out include/pixie_hip.h equal the ctypes mirror"""
    from pixie_amd import _lib
    header = os.path.join(os.path.dirname(HERE), "include", "pixie_hip.h")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(pixie_part_seg_desc));', 'printf("counts %d\\n", PIXIE_PART_SEG_COUNTS);']
    lines += [f'printf("{f} %zu\\n", offsetof(pixie_part_seg_desc, {f}));' for f, _ in _lib.PartSegDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_lib.PartSegDesc) and int(got["counts"]) == _lib.PART_SEG_COUNTS
    for f, _ in _lib.PartSegDesc._fields_:
        assert int(got[f]) == getattr(_lib.PartSegDesc, f).offset, f
