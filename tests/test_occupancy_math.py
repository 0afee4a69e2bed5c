"""CPU checks of pixie_amd/csrc/occupancy_math.h (compiled for the host by tests/host_harness/occupancy_math_host.cpp, g++
-ffp-contract=off): the occupancy mask through the same offset-table, cube-bisection and open-ball path as the kernels of
occupancy.hip, against the NumPy / scipy restatement of tests/_occupancy_ref.py.

Bars.  Bitmaps, masks, counts and the cluster count are EQUAL.  |m_i - ref| <= 4 E + 1e-12, E the largest float64 deviation of an
axis coordinate from the uniform lattice through the axis' end points: a neighbour's coordinate differences are each off the
lattice's by at most 2 E, so its distance by at most 2 sqrt(3) E < 4 E, which covers the one freedom the header has against the k-d
tree -- which members of the last shell it takes -- and 1e-12 covers the order of a 50-term float64 sum.  On the exact lattices E = 0.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _occupancy_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "occupancy_math_host.cpp")
FP, DP, U8, I32, I64 = (C.POINTER(t) for t in (C.c_float, C.c_double, C.c_uint8, C.c_int32, C.c_int64))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("occ_host") / "liboccupancy_math_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_occ_offsets.argtypes = [C.POINTER(C.c_int8)]
    h.hh_occ_mask.argtypes = [C.c_int] * 3 + [FP] * 5 + [C.c_double] * 4 + [C.c_int, C.c_double, C.c_int, C.c_double,
                                                                             U8, DP, U8, I32, U8, U8, I64, DP]
    return h


def host_mask(h, scene, lattice_spacing=None, **params):
    p = dict(R.DEFAULTS, **params)
    d, hh, w = scene["shape"]
    a = np.ascontiguousarray(scene["alphas"].reshape(d, hh, w), np.float32)
    c = np.ascontiguousarray(scene["rgb"], np.float32)
    ax, ay, az = (np.ascontiguousarray(x, np.float32) for x in scene["axes"])
    n = d * hh * w
    out = dict(cand=np.zeros(n, np.uint8), m=np.zeros(n, np.float64), stage_b=np.zeros(n, np.uint8), root=np.zeros(n, np.int32),
               non_noise=np.zeros(n, np.uint8), largest=np.zeros(n, np.uint8), counts=np.zeros(8, np.int64), stats=np.zeros(3, np.float64))
    rc = h.hh_occ_mask(d, hh, w, a.ctypes.data_as(FP), c.ctypes.data_as(FP), ax.ctypes.data_as(FP), ay.ctypes.data_as(FP), az.ctypes.data_as(FP),
                       scene["voxel_size"], lattice_spacing or scene["voxel_size"], p["alpha_threshold"], p["gray_threshold"], p["nb_neighbors"],
                       p["std_ratio"], p["min_cluster_pts"], p["eps_multiplier"], out["cand"].ctypes.data_as(U8), out["m"].ctypes.data_as(DP),
                       out["stage_b"].ctypes.data_as(U8), out["root"].ctypes.data_as(I32), out["non_noise"].ctypes.data_as(U8),
                       out["largest"].ctypes.data_as(U8), out["counts"].ctypes.data_as(I64), out["stats"].ctypes.data_as(DP))
    assert rc == 0
    for k in ("cand", "stage_b", "non_noise", "largest"):
        out[k] = out[k].reshape(d, hh, w).astype(bool)
    out["m"] = out["m"].reshape(d, hh, w)
    out["root"] = out["root"].reshape(d, hh, w)
    return out


def compare(got, ref, scene):
    """every voxel of every stage; shared with nothing: the GPU tests have their own copy of the same comparisons"""
    bar = 4.0 * R.lattice_deviation(scene["axes"]) + 1e-12
    assert np.array_equal(got["cand"], ref["cand"])
    assert np.all(np.isnan(got["m"][~ref["cand"]]))
    err = np.abs(got["m"][ref["cand"]] - ref["m"])
    print(f"{scene['name']}: M {ref['n_gray']}, slow path {int(got['counts'][4])}, worst |m - ref| {err.max() if len(err) else 0.0:.3e}, bar {bar:.3e}")
    assert np.all(err <= bar)
    assert np.array_equal(got["stage_b"], ref["stage_b"])
    assert np.array_equal(got["non_noise"], ref["non_noise"])
    assert np.array_equal(got["largest"], ref["largest"])
    assert list(got["counts"][:4]) == [ref["n_density"], ref["n_gray"], ref["n_stage_b"], int(ref["non_noise"].sum())]
    assert int(got["counts"][5]) == ref["n_clusters"]
    if ref["n_gray"] > 2:
        assert got["stats"] == pytest.approx([ref["cloud_mean"], ref["std"], ref["threshold"]], rel=1e-12, abs=bar)
    # the partition: voxels share a root iff they share a label, and roots ascend with the labels
    roots = got["root"][ref["stage_b"]]
    assert np.array_equal(roots >= 0, ref["labels"] >= 0)
    uniq = np.unique(roots[roots >= 0])
    assert np.array_equal(np.searchsorted(uniq, roots[roots >= 0]), ref["labels"][ref["labels"] >= 0])


SCENES = ["tiny16", "inexact24", "slab", "word70"]


@pytest.mark.parametrize("params", [R.DEFAULTS, R.OTHER], ids=["defaults", "other"])
@pytest.mark.parametrize("name", SCENES)
def test_header_equals_the_restatement(host, name, params):
    scene = R.build_scene(name)
    compare(host_mask(host, scene, **params), R.reference(scene, **params), scene)


@pytest.mark.parametrize("name", list(R.EDGE_SPACING))
def test_edge_scenes_where_pairs_at_exactly_eps_decide(host, name):
    """outcomes that a closed ball or an integer-offset comparison would change (tests/test_occupancy_ref.py shows that they do);
    float32 inputs one step either side of the thresholds"""
    scene = R.edge_scene(name)
    ref = R.reference(scene, **R.EDGE)
    compare(host_mask(host, scene, **R.EDGE), ref, scene)
    assert np.array_equal(ref["cand"], scene["structure"])


@pytest.mark.parametrize("params", [R.DEFAULTS, R.OTHER], ids=["defaults", "other"])
@pytest.mark.parametrize("count", [7, 2, 1, 0])
def test_few_candidates(host, count, params):
    scene = R.few_scene(count)
    got, ref = host_mask(host, scene, **params), R.reference(scene, **params)
    compare(got, ref, scene)
    if count <= 2:
        assert not got["stage_b"].any() and not got["non_noise"].any() and not got["largest"].any()
    if count == 2:
        assert got["stats"][1] == 0.0                                # std = 0 and the comparison is strict
    if count == 1:
        assert got["m"][got["cand"]][0] == 0.0 and np.isnan(got["stats"][1])


def test_tiny16_leaves_the_fast_path_and_ties_do_not_move_exact_lattices(host):
    scene = R.build_scene("tiny16")
    got = host_mask(host, scene)
    assert got["counts"][4] > 0.5 * got["counts"][1], "tiny16 is there to run the cube bisection"
    ref = R.reference(scene)
    assert np.max(np.abs(got["m"][ref["cand"]] - ref["m"])) <= 1e-12


def test_offset_table_is_every_offset_up_to_nine_in_ascending_shells(host):
    buf = (C.c_int8 * (4 * 128))()
    n = host.hh_occ_offsets(buf)
    t = np.frombuffer(buf, np.int8).reshape(128, 4)[:n].astype(int)
    assert n == 123
    assert np.array_equal((t[:, :3] ** 2).sum(axis=1), t[:, 3])
    assert np.all(np.diff(t[:, 3]) >= 0) and t[0].tolist() == [0, 0, 0, 0]
    assert len({tuple(r[:3]) for r in t}) == 123
    r = np.arange(-3, 4)
    assert n == int(((r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2) <= 9).sum())


def test_a_coarser_lattice_than_voxel_size_widens_nothing(host):
    """compute_occupancy_point_cloud clusters with eps = 5 * 0.01 on a lattice of spacing 1 / 63: the index neighbourhood follows
    eps / lattice_spacing, the comparison follows eps"""
    scene = dict(R.build_scene("inexact24"))
    spacing = scene["voxel_size"]
    scene["voxel_size"] = 0.6 * spacing                             # eps = 3 lattice spacings
    got = host_mask(host, scene, lattice_spacing=spacing)
    compare(got, R.reference(scene), scene)


def test_descriptor_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of pixie_occupancy_desc as gcc lays out include/pixie_hip.h equal the ctypes mirror"""
    from pixie_amd import _lib
    header = os.path.join(os.path.dirname(HERE), "include", "pixie_hip.h")
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void) {",
             'printf("size %zu\\n", sizeof(pixie_occupancy_desc));']
    lines += [f'printf("{f} %zu\\n", offsetof(pixie_occupancy_desc, {f}));' for f, _ in _lib.OccupancyDesc._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_lib.OccupancyDesc)
    for f, _ in _lib.OccupancyDesc._fields_:
        assert int(got[f]) == getattr(_lib.OccupancyDesc, f).offset, f
