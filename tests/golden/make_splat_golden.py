#!/usr/bin/env python
"""Writes tests/golden/splat_export.npz: the per-frame splat export of gs_simulation.py (export_gaussians_to_ply, :290-322)
computed by the REFERENCE's own code, for tests/test_splat_math.py, test_splat_ply.py and test_splat_export_hip.py.

1. Decomposition.  `cov3D_to_log_scales_and_quats` (gs_simulation.py:253-288) is cut out with `ast` and run unmodified on CPU torch
   (float32 and float64) with scipy, on
     * "frame": frame_export.npz's cov_f32 -- the reference's own compute_cov_from_F covariances in the world frame (150 Gaussians);
     * "synth": a synthetic set: isotropic, two equal eigenvalues (both ways round), anisotropy ratios 1e2 / 1e4 / 1e6, an
       eigenvalue under the 1e-12 clamp, everything under the clamp, and random spectra, under random rotations (float32 inputs).
   Recorded per set: the float32 input, the reference's outputs at float32 and float64, and a float64 numpy eigh of the input.
2. PLY layout.  GaussianModel.construct_list_of_attributes and save_ply (gaussian-splatting/scene/gaussian_model.py:177-208) are
   cut out and bound to a small stub object, with recording stand-ins for plyfile's PlyElement / PlyData, and run on tiny fixed
   inputs at SH degrees 0 and 3: the attribute name list and the structured array save_ply would have written are recorded.
Build container only (needs the reference tree and scipy); only data is committed.
"""
import ast
import os
import types

import numpy as np
import torch
from scipy.spatial.transform import Rotation as scipy_R

REF = "/root/reference/third_party/PhysGaussian"
HERE = os.path.dirname(os.path.abspath(__file__))


def cut_functions(path, names, ns, cls=None):
    tree = ast.parse(open(path).read())
    scope = tree.body
    if cls is not None:
        scope = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls).body
    body = [n for n in scope if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names), (path, names)
    exec(compile(ast.fix_missing_locations(ast.Module(body=body, type_ignores=[])), path, "exec"), ns)


def synthetic(rng):
    """(n, 6) float32 covariances from chosen spectra under random rotations (upper triangle s11 s12 s13 s22 s23 s33)"""
    spectra = []
    for a in (1e-2, 1e-4, 3e-6):
        spectra += [(a, a, a), (a, a, 0.3 * a), (a, 0.3 * a, 0.3 * a), (a, 1e-1 * a, 1e-2 * a), (a, 1e-2 * a, 1e-4 * a),
                    (a, 1e-3 * a, 1e-6 * a), (a, 0.5 * a, 1e-14)]
    spectra += [(1e-13, 5e-14, 1e-15), (1e-3, 1e-3 * (1 + 1e-6), 2e-4), (1e-3, 4e-4, -1e-9)]
    spectra += [tuple(10.0 ** rng.uniform(-7, -2, 3)) for _ in range(40)]
    out = []
    for k, lam in enumerate(spectra):
        R = scipy_R.random(random_state=int(rng.integers(1 << 30))).as_matrix()
        if k % 7 == 0 and k < 21:
            R = np.eye(3)                 # exactly diagonal inputs too
        S = R @ np.diag(lam) @ R.T
        out.append([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]])
    return np.asarray(out, np.float64).astype(np.float32)


def eigh64(c6):
    c = c6.astype(np.float64)
    S = np.stack([c[:, [0, 1, 2]], c[:, [1, 3, 4]], c[:, [2, 4, 5]]], axis=1)
    w, v = np.linalg.eigh(S)
    return w[:, ::-1].copy(), v[:, :, ::-1].copy()


class _Recorder:
    last = None


class PlyElement:
    @staticmethod
    def describe(elements, name):
        _Recorder.last = (name, elements.copy())
        return _Recorder.last


class PlyData:
    def __init__(self, els):
        self.els = els

    def write(self, path):
        pass


def main():
    ns = {"torch": torch, "np": np, "scipy_R": scipy_R}
    cut_functions(f"{REF}/gs_simulation.py", ["cov3D_to_log_scales_and_quats"], ns)
    decomp = ns["cov3D_to_log_scales_and_quats"]
    rng = np.random.default_rng(20261016)
    fe = np.load(os.path.join(HERE, "frame_export.npz"))
    out = {}
    for tag, c6 in (("frame", fe["cov_f32"].astype(np.float32)), ("synth", synthetic(rng))):
        out[f"{tag}/cov"] = c6
        for dname, dt in (("f32", torch.float32), ("f64", torch.float64)):
            ls, q = decomp(torch.tensor(c6.astype(np.float64), dtype=dt))
            out[f"{tag}/ref_{dname}_log_scale"] = ls.numpy()
            out[f"{tag}/ref_{dname}_quat"] = q.numpy()
        w, v = eigh64(c6)
        out[f"{tag}/eigh64_w"], out[f"{tag}/eigh64_v"] = w, v

    # PLY layout of GaussianModel.save_ply
    gm = {"np": np, "os": os, "PlyElement": PlyElement, "PlyData": PlyData, "mkdir_p": lambda p: None}
    cut_functions(f"{REF}/gaussian-splatting/scene/gaussian_model.py", ["construct_list_of_attributes", "save_ply"], gm, cls="GaussianModel")
    for deg in (0, 3):
        k = (deg + 1) ** 2
        n = 5
        g = np.random.default_rng(100 + deg)
        xyz = g.normal(size=(n, 3)).astype(np.float32)
        shs = g.normal(size=(n, k, 3)).astype(np.float32)
        opacity = g.uniform(0, 1, size=(n, 1)).astype(np.float32)
        scale = g.normal(-5, 1, size=(n, 3)).astype(np.float32)
        rot = g.normal(size=(n, 4)).astype(np.float32)
        stub = types.SimpleNamespace(_xyz=torch.from_numpy(xyz), _features_dc=torch.from_numpy(shs[:, :1, :]),
                                     _features_rest=torch.from_numpy(shs[:, 1:, :]), _opacity=torch.from_numpy(opacity),
                                     _scaling=torch.from_numpy(scale), _rotation=torch.from_numpy(rot))
        stub.construct_list_of_attributes = types.MethodType(gm["construct_list_of_attributes"], stub)
        gm["save_ply"](stub, "frame_00000.ply")
        name, elements = _Recorder.last
        assert name == "vertex"
        out.update({f"ply{deg}/xyz": xyz, f"ply{deg}/shs": shs, f"ply{deg}/opacity": opacity, f"ply{deg}/scale": scale,
                    f"ply{deg}/rot": rot, f"ply{deg}/names": np.array(stub.construct_list_of_attributes()), f"ply{deg}/elements": elements})
    np.savez_compressed(os.path.join(HERE, "splat_export.npz"), **out)
    print("wrote splat_export.npz:", {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
