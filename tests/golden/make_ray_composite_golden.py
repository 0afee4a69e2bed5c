"""Writes tests/golden/ray_composite.npz: the reference's own ray compositing functions, cut out of its source and run in float64.

    python tests/golden/make_ray_composite_golden.py <reference checkout>

The reference's modules do not import here (jaxtyping and nerfacc are absent), so the functions are cut out with `ast`: the method
definitions of RaySamples.get_weights, RGBRenderer.combine_rgb / get_background_color, AccumulationRenderer.forward,
DepthRenderer.forward (both branches) and f3rm's FeatureRenderer.forward, with their annotations stripped, compiled into bare classes
and run on the CPU with float64 as torch's default dtype.  The fixture holds the inputs (R = 8, S = 12, C = 8) and the outputs: data
only.  tests/test_ray_render_math.py compares tests/_ray_render_ref.py with it to 1e-14.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ray_render_ref as ref  # noqa: E402

CUTS = (("third_party/nerfstudio/nerfstudio/cameras/rays.py", "RaySamples", ("get_weights",)),
        ("third_party/nerfstudio/nerfstudio/model_components/renderers.py", "RGBRenderer", ("combine_rgb", "get_background_color")),
        ("third_party/nerfstudio/nerfstudio/model_components/renderers.py", "AccumulationRenderer", ("forward",)),
        ("third_party/nerfstudio/nerfstudio/model_components/renderers.py", "DepthRenderer", ("forward",)),
        ("third_party/f3rm/f3rm/renderer.py", "FeatureRenderer", ("forward",)))


def cut(root, path, cls, names, namespace):
    tree = ast.parse(open(os.path.join(root, path)).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    funcs = []
    for f in node.body:
        if isinstance(f, ast.FunctionDef) and f.name in names and not any(getattr(d, "id", "") == "overload" for d in f.decorator_list):
            f.returns = None
            for a in f.args.posonlyargs + f.args.args + f.args.kwonlyargs + [x for x in (f.args.vararg, f.args.kwarg) if x]:
                a.annotation = None
            f.decorator_list = [d for d in f.decorator_list if getattr(d, "id", "") == "classmethod"]
            funcs.append(f)
    assert sorted(f.name for f in funcs) == sorted(names), (cls, [f.name for f in funcs])
    module = ast.Module(body=[ast.ClassDef(name=cls, bases=[], keywords=[], body=funcs, decorator_list=[])], type_ignores=[])
    exec(compile(ast.fix_missing_locations(module), path, "exec"), namespace)
    return namespace[cls]


def main(root):
    torch.set_default_dtype(torch.float64)
    colors = types.SimpleNamespace(COLORS_DICT={"white": torch.tensor([1.0, 1.0, 1.0]), "black": torch.tensor([0.0, 0.0, 0.0])})
    ns = {"torch": torch, "Tensor": torch.Tensor, "nerfacc": None, "colors": colors, "BACKGROUND_COLOR_OVERRIDE": None}
    classes = {cls: cut(root, path, cls, names, ns) for path, cls, names in CUTS}
    inp = ref.make_inputs(8, 12, 8, seed=2024)
    inp["densities"][3] = 0.0                                       # an empty ray: full background, depth clipped to the global minimum
    t = {k: torch.tensor(v, dtype=torch.float64) for k, v in inp.items()}
    samples = classes["RaySamples"]()
    samples.deltas = t["deltas"]
    samples.frustums = types.SimpleNamespace(starts=t["starts"], ends=t["ends"])
    w = samples.get_weights(t["densities"])
    depth = lambda method: (lambda r: (setattr(r, "method", method), r.forward(w, samples))[1])(classes["DepthRenderer"]())
    out = {"weights": w, "accumulation": classes["AccumulationRenderer"].forward(w), "median_depth": depth("median"),
           "expected_depth": depth("expected"), "feature": classes["FeatureRenderer"].forward(t["features"], w)}
    for bg in ("random", "last_sample", "white"):
        out["rgb_" + bg] = classes["RGBRenderer"].combine_rgb(t["rgb"], w, background_color=bg)
    arrays = {k: v.numpy() for k, v in t.items()}
    arrays.update({"out_" + k: v.numpy() for k, v in out.items()})
    np.savez_compressed(os.path.join(HERE, "ray_composite.npz"), **arrays)
    print({k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main(sys.argv[1])
