"""CPU checks of pixie_amd/csrc/splat_math.h (compiled for the host by tests/host_harness/splat_math_host.cpp, g++
-ffp-contract=off) against the reference's cov3D_to_log_scales_and_quats recorded in tests/golden/splat_export.npz."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _splat_checks as sc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "splat_math_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("splat_host") / "libsplat_math_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_splat_from_cov.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]

    def run(c6):
        c6 = np.ascontiguousarray(c6, np.float32)
        ls = np.empty((len(c6), 3), np.float32)
        q = np.empty((len(c6), 4), np.float32)
        h.hh_splat_from_cov(len(c6), c6.ctypes.data, ls.ctypes.data, q.ctypes.data)
        return ls, q
    return run


@pytest.mark.parametrize("tag", ["frame", "synth"])
def test_splat_from_cov_meets_the_bars(host, tag):
    g = sc.golden()
    c6 = g[f"{tag}/cov"]
    ls, q = host(c6)
    checked, e_lam, e_rec = sc.check_splats(c6, ls, q, g[f"{tag}/eigh64_w"], g[f"{tag}/eigh64_v"], g[f"{tag}/ref_f32_log_scale"],
                                            g[f"{tag}/ref_f32_quat"], what=tag)
    assert checked > len(c6)       # most eigenvectors are separated and so were compared
    print(f"{tag}: eigenvalue err {e_lam:.2e}, reconstruction err {e_rec:.2e} (of lambda_1), {checked} eigenvectors compared")


def test_log_scales_match_the_float64_reference():
    """the reference's own float64 run (its clamp, sort and log) gives the same log-scales to float32 rounding"""
    g = sc.golden()
    for tag in ("frame", "synth"):
        ls = g[f"{tag}/ref_f64_log_scale"]
        w = g[f"{tag}/eigh64_w"]
        assert np.allclose(ls, 0.5 * np.log(np.maximum(w, sc.CLAMP)), rtol=0, atol=1e-6), tag


def test_degenerate_and_signs(host):
    """isotropic, two-equal, zero and diagonal inputs: finite, unit, right-handed; a diagonal input with distinct eigenvalues
    gives a permutation matrix with the documented signs (largest component of columns 0, 1 positive)"""
    c6 = np.array([[1e-4, 0, 0, 1e-4, 0, 1e-4],        # isotropic
                   [2e-4, 0, 0, 1e-4, 0, 1e-4],        # two equal
                   [0, 0, 0, 0, 0, 0],                 # zero
                   [1e-6, 0, 0, 3e-6, 0, 2e-6]], np.float32)
    ls, q = host(c6)
    assert np.isfinite(ls).all() and np.isfinite(q).all()
    assert np.allclose(np.linalg.norm(q.astype(np.float64), axis=1), 1.0, atol=1e-6) and (q[:, 0] >= 0).all()
    R = sc.quat_to_R(q)
    assert np.allclose(np.linalg.det(R), 1.0, atol=1e-6)
    assert np.allclose(ls[2], 0.5 * np.log(1e-12), atol=1e-6)
    assert np.allclose(R[3], [[0, 0, 1], [1, 0, 0], [0, 1, 0]], atol=1e-6)   # columns e_y (3e-6), e_z (2e-6), e_y x e_z = e_x
    for k in range(4):
        for c in (0, 1):
            col = R[k, :, c]
            assert col[np.argmax(np.abs(col))] > 0
