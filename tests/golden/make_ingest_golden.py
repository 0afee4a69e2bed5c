#!/usr/bin/env python
"""Writes tests/golden/scene_ingest.npz and the input checkpoints tests/golden/ingest_<case>.ply: the span of gs_simulation.py in
front of fill_particles (:403-438) computed by the REFERENCE's own code, for tests/test_scene_ingest_math.py,
test_scene_ingest_ply.py and test_scene_ingest_hip.py.

Cut out with `ast` and run unmodified on CPU torch, with the device string "cuda" turned into "cpu" and `plyfile` supplied by a
stand-in over pixie_amd.ply_io.read_ply:
  * GaussianModel: setup_functions, __init__, the get_* accessors, get_covariance, load_ply (gaussian-splatting/scene/gaussian_model.py)
  * build_rotation, build_scaling_rotation, strip_lowerdiag, strip_symmetric (gaussian-splatting/utils/general_utils.py)
  * generate_rotation_matrix(es), apply_rotation(s), apply_cov_rotation(s), get_mat_from_upper, get_uppder_from_mat,
    transform2origin, shift2center111 and, for the round trip the frame export undoes, undoshift2center111, undotransform2origin,
    apply_inverse_rotation(s), apply_inverse_cov_rotations (utils/transformation_utils.py)
  * load_params_from_gs (utils/render_utils.py)
  * the statements of gs_simulation.py:403-438
at float32 (as the reference runs) and at float64 (torch's default dtype set to float64 and `torch.float` bound to it).

Inputs: synthetic checkpoints of a few hundred Gaussians.  Every Gaussian is kept at least 1e-4 away from both thresholds --
|sigmoid(opacity) - opacity_threshold| and the distance of every rotated coordinate from every sim_area face -- which is asserted on
both runs, so the classification of these inputs does not depend on float32 rounding.  Cases with a sim_area leave at least 20 % of
the Gaussians in each of the three classes; "deg0" has no sim_area and so no unselected Gaussian.
Recorded per case: the config, the float32 rotation matrices, the kept indices of both classes, the reference's outputs at both
precisions, and the error of its float32 export round trip (pos / cov back to the scene frame against the checkpoint's own values).
Build container only (needs the reference tree); only data is committed.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/third_party/PhysGaussian"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pixie_amd.ply_io import read_ply, write_ply_f4  # noqa: E402
from pixie_amd.splat_export import attribute_names  # noqa: E402

MARGIN = 1e-4

CASES = {
    "deg3": dict(n=300, sh_degree=3, seed=11, opacity_threshold=0.3, rotation_degree=[30.0, -75.0], rotation_axis=[0, 2],
                 sim_area=[-0.8, 0.75, -0.85, 0.7, -0.75, 0.8], z_shift_value=0.3),
    "deg0": dict(n=200, sh_degree=0, seed=12, opacity_threshold=0.25, rotation_degree=[], rotation_axis=[], sim_area=None,
                 z_shift_value=0.0),
    "rot3": dict(n=250, sh_degree=3, seed=13, opacity_threshold=0.35, rotation_degree=[12.0, 200.0, -41.5], rotation_axis=[1, 0, 2],
                 sim_area=[-0.75, 0.8, -0.7, 0.85, -0.8, 0.75], z_shift_value=0.0),
}


class CudaToCpu(ast.NodeTransformer):
    def visit_Constant(self, node):
        return ast.copy_location(ast.Constant("cpu"), node) if node.value in ("cuda", "cuda:0") else node

    def visit_Call(self, node):          # tensor.cuda() -> tensor
        self.generic_visit(node)
        if isinstance(node.func, ast.Attribute) and node.func.attr == "cuda" and not node.args:
            return node.func.value
        return node


def run_nodes(nodes, path, ns):
    mod = ast.fix_missing_locations(CudaToCpu().visit(ast.Module(body=list(nodes), type_ignores=[])))
    exec(compile(mod, path, "exec"), ns)


def cut(path, names, ns):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names), (path, names)
    run_nodes(body, path, ns)


def cut_class(path, cls, names, ns):
    tree = ast.parse(open(path).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    body = [n for n in node.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(body) == len(names), (path, names)
    run_nodes([ast.ClassDef(name=cls, bases=[], keywords=[], body=body, decorator_list=[])], path, ns)


def main_statements(path, first, last):
    """the statements of the `if __name__ == "__main__":` block whose lines lie in [first, last]"""
    tree = ast.parse(open(path).read())
    main = next(n for n in tree.body if isinstance(n, ast.If) and "__main__" in ast.dump(n.test))
    body = [n for n in main.body if first <= n.lineno and n.end_lineno <= last]
    assert body[0].lineno == first and body[-1].end_lineno == last, (body[0].lineno, body[-1].end_lineno)
    return body


class _Element:
    def __init__(self, vertex):
        self._vertex = vertex
        self.properties = [types.SimpleNamespace(name=n) for n in vertex.dtype.names]

    def __getitem__(self, name):
        return self._vertex[name]


class PlyData:
    """plyfile.PlyData.read as load_ply uses it: elements[0][name] and elements[0].properties[i].name"""

    @staticmethod
    def read(path):
        return types.SimpleNamespace(elements=[_Element(read_ply(path)[0])])


class TorchAt:
    """the torch module with `torch.float` bound to the run's precision"""

    def __init__(self, dt):
        self._dt = dt

    def __getattr__(self, name):
        return self._dt if name == "float" else getattr(torch, name)


def namespace(dt):
    t = TorchAt(dt)
    ns = {"torch": t, "np": np, "nn": torch.nn, "os": os, "PlyData": PlyData, "inverse_sigmoid": None, "print": lambda *a, **k: None}
    cut(f"{REF}/gaussian-splatting/utils/general_utils.py", ["strip_lowerdiag", "strip_symmetric", "build_rotation", "build_scaling_rotation"], ns)
    cut_class(f"{REF}/gaussian-splatting/scene/gaussian_model.py", "GaussianModel",
              ["setup_functions", "__init__", "get_scaling", "get_rotation", "get_xyz", "get_features", "get_opacity", "get_covariance", "load_ply"], ns)
    cut(f"{REF}/utils/transformation_utils.py",
        ["transform2origin", "undotransform2origin", "generate_rotation_matrix", "generate_rotation_matrices", "apply_rotation",
         "apply_cov_rotation", "get_mat_from_upper", "get_uppder_from_mat", "apply_rotations", "apply_cov_rotations", "shift2center111",
         "undoshift2center111", "apply_inverse_rotation", "apply_inverse_rotations", "apply_inverse_cov_rotations"], ns)
    cut(f"{REF}/utils/render_utils.py", ["load_params_from_gs"], ns)
    return ns


def make_checkpoint(case, path):
    """a synthetic checkpoint whose Gaussians all keep MARGIN from the case's thresholds (checked again on the reference's values)"""
    rng = np.random.default_rng(case["seed"])
    n, k = case["n"], (case["sh_degree"] + 1) ** 2
    R = np.eye(3)
    for deg, ax in zip(case["rotation_degree"], case["rotation_axis"]):
        a = deg / 180.0 * 3.1415926
        c, s = np.cos(a), np.sin(a)
        m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[ax]
        R = np.asarray(m) @ R
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    raw = rng.normal(0.0, 2.0, n).astype(np.float32)
    for _ in range(100):
        rp = xyz.astype(np.float64) @ R.T
        near = np.abs(1 / (1 + np.exp(-raw.astype(np.float64))) - case["opacity_threshold"]) < 10 * MARGIN
        if case["sim_area"] is not None:
            near |= (np.abs(rp[:, [0, 0, 1, 1, 2, 2]] - np.asarray(case["sim_area"])) < 10 * MARGIN).any(axis=1)
        if not near.any():
            break
        xyz[near] = rng.uniform(-1, 1, (int(near.sum()), 3)).astype(np.float32)
        raw[near] = rng.normal(0.0, 2.0, int(near.sum())).astype(np.float32)
    assert not near.any()
    shs = rng.normal(0, 0.5, (n, k, 3)).astype(np.float32)
    block = np.concatenate([xyz, np.zeros((n, 3), np.float32), shs[:, :1].transpose(0, 2, 1).reshape(n, -1),
                            shs[:, 1:].transpose(0, 2, 1).reshape(n, -1), raw[:, None],
                            rng.normal(-4.0, 0.7, (n, 3)).astype(np.float32), rng.normal(0, 1, (n, 4)).astype(np.float32)], axis=1)
    write_ply_f4(path, attribute_names(k), block)


def run_reference(case, path, dt, statements):
    torch.set_default_dtype(dt)
    ns = namespace(dt)
    gaussians = ns["GaussianModel"](case["sh_degree"])
    gaussians.load_ply(path)
    ns.update(gaussians=gaussians, pipeline=types.SimpleNamespace(compute_cov3D_python=True, convert_SHs_python=False, debug=False),
              preprocessing_params={k: case[k] for k in ("opacity_threshold", "rotation_degree", "rotation_axis", "sim_area", "z_shift_value")})
    run_nodes(statements, f"{REF}/gs_simulation.py", ns)
    # the export round trip of the frame loop (:591-600) at step 0, the reference's own functions
    ns["back_pos"] = ns["apply_inverse_rotations"](ns["undotransform2origin"](ns["undoshift2center111"](
        ns["transformed_pos"], case["z_shift_value"]), ns["scale_origin"], ns["original_mean_pos"]), ns["rotation_matrices"])
    ns["back_cov"] = ns["apply_inverse_cov_rotations"](ns["init_cov"] / (ns["scale_origin"] ** 2), ns["rotation_matrices"])
    torch.set_default_dtype(torch.float32)
    return ns


def np_(t):
    return t.detach().cpu().numpy()


def main():
    statements = main_statements(f"{REF}/gs_simulation.py", 403, 438)
    out = {}
    report = []
    for name, case in CASES.items():
        path = os.path.join(HERE, f"ingest_{name}.ply")
        make_checkpoint(case, path)
        runs = {tag: run_reference(case, path, dt, statements) for tag, dt in (("f32", torch.float32), ("f64", torch.float64))}
        n = case["n"]
        for tag, ns in runs.items():
            op = np_(ns["params"]["opacity"])[:, 0].astype(np.float64)
            assert (np.abs(op - case["opacity_threshold"]) >= MARGIN).all(), (name, tag)
            kept = np.flatnonzero(op > case["opacity_threshold"])
            rp = np_(ns["apply_rotations"](ns["params"]["pos"][torch.as_tensor(kept)], ns["rotation_matrices"])).astype(np.float64)
            if case["sim_area"] is not None:
                assert (np.abs(rp[:, [0, 0, 1, 1, 2, 2]] - np.asarray(case["sim_area"])) >= MARGIN).all(), (name, tag)
                inside = np_(ns["mask"])
            else:
                inside = np.ones(len(kept), bool)
            sel, unsel = kept[inside], kept[~inside]
            assert len(sel) == ns["transformed_pos"].shape[0]
            out[f"{name}/{tag}/sel_index"], out[f"{name}/{tag}/unsel_index"] = sel, unsel
            out[f"{name}/{tag}/pos"] = np_(ns["transformed_pos"])
            out[f"{name}/{tag}/cov"] = np_(ns["init_cov"])
            out[f"{name}/{tag}/opacity"] = np_(ns["init_opacity"])
            out[f"{name}/{tag}/shs"] = np_(ns["init_shs"])
            out[f"{name}/{tag}/scale_origin"] = np_(ns["scale_origin"])
            out[f"{name}/{tag}/original_mean_pos"] = np_(ns["original_mean_pos"])
            out[f"{name}/{tag}/rotation_matrices"] = (np_(torch.stack(ns["rotation_matrices"])) if ns["rotation_matrices"]
                                                      else np.zeros((0, 3, 3), np_(ns["scale_origin"]).dtype))
            out[f"{name}/{tag}/all_xyz"] = np_(ns["params"]["pos"])
            out[f"{name}/{tag}/all_cov"] = np_(ns["params"]["cov3D_precomp"])
            out[f"{name}/{tag}/all_opacity"] = np_(ns["params"]["opacity"])
            out[f"{name}/{tag}/all_shs"] = np_(ns["params"]["shs"])
            if case["sim_area"] is not None:
                out[f"{name}/{tag}/unsel_pos"] = np_(ns["unselected_pos"])
                out[f"{name}/{tag}/unsel_cov"] = np_(ns["unselected_cov"])
                out[f"{name}/{tag}/unsel_opacity"] = np_(ns["unselected_opacity"])
                out[f"{name}/{tag}/unsel_shs"] = np_(ns["unselected_shs"])
                fr = np.array([len(sel), len(unsel), n - len(kept)]) / n
                assert (fr >= 0.2).all(), (name, fr)
            out[f"{name}/{tag}/roundtrip_pos"], out[f"{name}/{tag}/roundtrip_cov"] = np_(ns["back_pos"]), np_(ns["back_cov"])
        for key in ("sel_index", "unsel_index"):
            assert np.array_equal(out[f"{name}/f32/{key}"], out[f"{name}/f64/{key}"]), (name, key)
        out[f"{name}/config"] = np.array(repr({k: v for k, v in case.items() if k not in ("n", "seed")}))
        ys = {q: rel(out[f"{name}/f32/{q}"], out[f"{name}/f64/{q}"]) for q in ("pos", "cov", "opacity", "scale_origin", "original_mean_pos")
              + (("unsel_cov", "unsel_opacity") if case["sim_area"] is not None else ())}
        sel = out[f"{name}/f64/sel_index"]
        ys["roundtrip_pos"] = rel(out[f"{name}/f32/roundtrip_pos"], out[f"{name}/f64/all_xyz"][sel])
        ys["roundtrip_cov"] = rel(out[f"{name}/f32/roundtrip_cov"], out[f"{name}/f64/all_cov"][sel])
        report.append((name, len(sel), len(out[f"{name}/f64/unsel_index"]), ys))
    np.savez_compressed(os.path.join(HERE, "scene_ingest.npz"), **out)
    for name, ns_, nu, ys in report:
        print(f"{name}: {ns_} selected, {nu} unselected; reference float32 vs float64 (max-abs over max-abs):",
              ", ".join(f"{k} {v:.2e}" for k, v in ys.items()))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


if __name__ == "__main__":
    main()
