"""CPU checks of pixie_amd/csrc/ingest_math.h (compiled for the host by tests/host_harness/ingest_math_host.cpp, g++
-ffp-contract=off) against the reference's own run of gs_simulation.py:403-438 recorded in tests/golden/scene_ingest.npz, and of
the NumPy restatement tests/_ingest_ref.py that the GPU tests use at other sizes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pixie_amd.scene_ingest import generate_rotation_matrices, load_gaussian_ply
from tests import _ingest_ref as ir

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "ingest_math_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("ingest_host") / "libingest_math_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_ingest.argtypes = ([C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                             C.c_float] + [C.c_void_p] * 8)

    def run(block, columns, k, cfg):
        """(return code, dict with the golden's keys)"""
        block = np.ascontiguousarray(block, np.float32)
        n = block.shape[0]
        mats = generate_rotation_matrices(cfg.get("rotation_degree", []), cfg.get("rotation_axis", []))
        rot = np.ascontiguousarray(np.stack([m.numpy() for m in mats]).reshape(-1) if mats else np.zeros(9), np.float32)
        area = np.asarray(cfg["sim_area"] if cfg.get("sim_area") is not None else [0] * 6, np.float32)
        columns = np.ascontiguousarray(columns, np.int32)
        cls = np.zeros(n, np.int32)
        pos, cov, op, shs = (np.zeros((n, 3), np.float32), np.zeros((n, 6), np.float32), np.zeros((n, 1), np.float32),
                             np.zeros((n, k, 3), np.float32))
        counts, scale, mean = np.zeros(3, np.int64), np.zeros(1, np.float32), np.zeros(3, np.float32)
        rc = h.hh_ingest(n, block.shape[1], block.ctypes.data, columns.ctypes.data, k, len(mats), rot.ctypes.data,
                         int(cfg.get("sim_area") is not None), area.ctypes.data, cfg["opacity_threshold"], cfg.get("z_shift_value", 0.0),
                         cls.ctypes.data, pos.ctypes.data, cov.ctypes.data, op.ctypes.data, shs.ctypes.data, counts.ctypes.data,
                         scale.ctypes.data, mean.ctypes.data)
        ns, nu = int(counts[0]), int(counts[1])
        return rc, dict(sel_index=np.flatnonzero(cls == 1), unsel_index=np.flatnonzero(cls == 2), pos=pos[:ns], cov=cov[:ns],
                        opacity=op[:ns], shs=shs[:ns], unsel_pos=pos[ns:ns + nu], unsel_cov=cov[ns:ns + nu],
                        unsel_opacity=op[ns:ns + nu], unsel_shs=shs[ns:ns + nu], scale_origin=scale[0], original_mean_pos=mean,
                        counts=counts)
    return run


@pytest.mark.parametrize("case", ir.CASES)
def test_header_meets_the_bars_on_the_golden(host, case):
    ck = load_gaussian_ply(ir.golden_ply(case), ir.golden_config(case)["sh_degree"])
    _, f64, y = ir.golden_runs(case)
    rc, got = host(ck.block, ck.columns, ck.n_sh_coeffs, ir.golden_config(case))
    assert rc == 0
    assert list(got["counts"]) == [len(f64["sel_index"]), len(f64["unsel_index"]), len(ck) - len(f64["sel_index"]) - len(f64["unsel_index"])]
    ir.check_against(got, f64, y, f"host {case}")


@pytest.mark.parametrize("case", ir.CASES)
def test_numpy_restatement_is_pinned_to_the_golden(case):
    """float64 restatement == the reference's float64 run to rounding; the float32 one lies as close to the float64 run as the
    reference's own float32 run does (same bar); margins of the inputs are as the generator promises"""
    cfg = ir.golden_config(case)
    ck = load_gaussian_ply(ir.golden_ply(case), cfg["sh_degree"])
    f32, f64, y = ir.golden_runs(case)
    r64 = ir.reference(ck.block, ck.columns, ck.n_sh_coeffs, cfg, np.float64)
    assert r64["opacity_margin"] >= ir.MARGIN and r64["rotated_margin"] >= ir.MARGIN
    for key in ("sel_index", "unsel_index"):
        assert np.array_equal(r64[key], f64[key])
    for q in ir.FLOATING + ("unsel_pos",):
        if q in f64:
            assert ir.rel(r64[q], f64[q]) < 1e-13, q
    assert np.array_equal(r64["shs"], f64["shs"]) and np.array_equal(r64["all_cov"].shape, f64["all_cov"].shape)
    mats = [m.numpy() for m in generate_rotation_matrices(cfg["rotation_degree"], cfg["rotation_axis"])]
    r32 = ir.reference(ck.block, ck.columns, ck.n_sh_coeffs, cfg, np.float32, mats=mats)
    ir.check_against(r32, f64, y, f"numpy float32 {case}")
    frac = np.array([len(f64["sel_index"]), len(f64["unsel_index"]), len(ck) - len(f64["sel_index"]) - len(f64["unsel_index"])]) / len(ck)
    if cfg["sim_area"] is not None:
        assert (frac >= 0.2).all(), frac


def test_longest_axis_spans_half_to_one_and_a_half_exactly(host):
    """the box and the mapped positions come from the same rotated positions: min 0.5 and max 1.5 on the longest axis, before the
    z shift"""
    for case in ir.CASES:
        cfg = dict(ir.golden_config(case), z_shift_value=0.0)
        ck = load_gaussian_ply(ir.golden_ply(case), cfg["sh_degree"])
        rc, got = host(ck.block, ck.columns, ck.n_sh_coeffs, cfg)
        assert rc == 0
        ext = got["pos"].max(axis=0) - got["pos"].min(axis=0)
        ax = int(np.argmax(ext))
        assert got["pos"][:, ax].min() == np.float32(0.5) and got["pos"][:, ax].max() == np.float32(1.5), case


def test_refusals_and_two_survivors(host):
    cfg = dict(opacity_threshold=0.3, rotation_degree=[20.0], rotation_axis=[1], sim_area=None, z_shift_value=0.0)
    block, _names = ir.synthetic_block(50, 1, 5, cfg, keep_only=2)
    from pixie_amd.scene_ingest import GaussianCheckpoint
    ck = GaussianCheckpoint(block, _names, 0)
    rc, got = host(ck.block, ck.columns, 1, cfg)
    assert rc == 0 and list(got["counts"]) == [2, 0, 48]
    one, _ = ir.synthetic_block(50, 1, 5, cfg, keep_only=1)
    assert host(one, ck.columns, 1, cfg)[0] == 3                                               # zero extent
    assert host(block, ck.columns, 1, dict(cfg, sim_area=[5, 6, 5, 6, 5, 6]))[0] == 2           # nothing selected
    none, _ = ir.synthetic_block(50, 1, 5, cfg, keep_only=0)
    assert host(none, ck.columns, 1, cfg)[0] == 2
