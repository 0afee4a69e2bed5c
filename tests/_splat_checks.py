"""Bars for the covariance -> (log-scale, quaternion) decomposition against tests/golden/splat_export.npz, shared by the host
(test_splat_math.py) and device (test_splat_export_hip.py) tests.  TEST INFRASTRUCTURE ONLY."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "splat_export.npz")
CLAMP = 1e-12


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def quat_to_R(q):
    """(n, 4) wxyz -> (n, 3, 3) rotation matrices (float64), normalised"""
    q = np.asarray(q, np.float64)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], axis=1)


def sym(c6):
    c = np.asarray(c6, np.float64)
    return np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)


def errors(c6, ls, q, w64):
    """per Gaussian: eigenvalue error max_i |exp(2 ls_i) - max(lambda_i, 1e-12)| and reconstruction error max |R diag R^T - S|
    (NaN where a clamp applies), both over the scale max(lambda_1, 1e-12)"""
    scale = np.maximum(w64[:, 0], CLAMP)
    lam = np.exp(2.0 * np.asarray(ls, np.float64))
    e_lam = np.abs(lam - np.maximum(w64, CLAMP)).max(axis=1) / scale
    R = quat_to_R(q)
    rec = np.einsum("nij,nj,nkj->nik", R, lam, R)
    e_rec = np.abs(rec - sym(c6)).reshape(-1, 9).max(axis=1) / scale
    e_rec[(w64 <= CLAMP).any(axis=1)] = np.nan
    return e_lam, e_rec


def check_splats(c6, ls, q, w64, v64, ref_ls32=None, ref_q32=None, what=""):
    """The bars of the issue (scale = max(lambda_1, 1e-12), lambda the float64 eigenvalues of the float32 input)."""
    ls, q = np.asarray(ls), np.asarray(q)
    assert ls.dtype == np.float32 and q.dtype == np.float32, what
    assert np.isfinite(ls).all() and np.isfinite(q).all(), what
    assert (np.diff(ls, axis=1) <= 0).all(), f"{what}: log-scales not descending"
    e_lam, e_rec = errors(c6, ls, q, w64)
    assert e_lam.max() <= 1e-6, (what, "eigenvalue", e_lam.max())
    assert np.nanmax(e_rec) <= 2e-6, (what, "reconstruction", np.nanmax(e_rec))
    q64 = q.astype(np.float64)
    assert np.abs(np.linalg.norm(q64, axis=1) - 1.0).max() <= 1e-6, what
    assert (q64[:, 0] >= 0).all(), f"{what}: w < 0"
    R = quat_to_R(q64)
    assert np.abs(np.linalg.det(R) - 1.0).max() <= 1e-6, what
    # eigenvectors where the eigenvalue is separated (relative gap >= 1e-2): within 1e-4 rad of float64 eigh, up to sign
    scale = np.maximum(w64[:, 0], CLAMP)
    checked = 0
    for i in range(3):
        gap = np.min([np.abs(w64[:, i] - w64[:, j]) for j in range(3) if j != i], axis=0) / scale
        sel = gap >= 1e-2
        s = np.linalg.norm(np.cross(R[sel, :, i], v64[sel, :, i]), axis=1)      # sin of the angle, sign-free
        assert (s <= 1e-4).all(), (what, "eigenvector", i, s.max())
        checked += int(sel.sum())
    # never further from float64 than the reference's float32 run, x1.5 + 1e-7
    if ref_ls32 is not None:
        r_lam, r_rec = errors(c6, ref_ls32, ref_q32, w64)
        assert e_lam.max() <= 1.5 * r_lam.max() + 1e-7, (what, e_lam.max(), r_lam.max())
        assert np.nanmax(e_rec) <= 1.5 * np.nanmax(r_rec) + 1e-7, (what, np.nanmax(e_rec), np.nanmax(r_rec))
    return checked, e_lam.max(), np.nanmax(e_rec)
