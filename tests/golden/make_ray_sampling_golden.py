"""Writes tests/golden/ray_sampling.npz: the reference's own PDF sampler and proposal losses, cut out of its source and run in float64.

    python tests/golden/make_ray_sampling_golden.py <reference checkout>

The reference's modules do not import here (jaxtyping and nerfacc are absent), so the functions are cut out with `ast`, as
make_ray_composite_golden.py does: PDFSampler.generate_ray_samples from ray_samplers.py, and outer, lossfun_outer, ray_samples_to_sdist,
interlevel_loss, lossfun_distortion and distortion_loss from losses.py, with their annotations stripped, compiled and run on the CPU
with float64 as torch's default dtype.  ray_bundle.get_ray_samples is a stub that records its arguments.  The fixture holds the inputs
(R = 8, 12 existing samples, 9 requested) and the outputs: data only.  tests/test_ray_sampling_math.py compares
tests/_ray_sampling_ref.py with it to 1e-14.
"""
import ast
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ray_sampling_ref as ref  # noqa: E402

SAMPLERS = "third_party/nerfstudio/nerfstudio/model_components/ray_samplers.py"
LOSSES = "third_party/nerfstudio/nerfstudio/model_components/losses.py"
LOSS_FUNCTIONS = ("outer", "lossfun_outer", "ray_samples_to_sdist", "interlevel_loss", "lossfun_distortion", "distortion_loss")


def strip(f):
    f.returns = None
    for a in f.args.posonlyargs + f.args.args + f.args.kwonlyargs + [x for x in (f.args.vararg, f.args.kwarg) if x]:
        a.annotation = None
    f.decorator_list = []
    return f


def cut_method(root, path, cls, name, namespace):
    tree = ast.parse(open(os.path.join(root, path)).read())
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls)
    funcs = [strip(f) for f in node.body if isinstance(f, ast.FunctionDef) and f.name == name]
    assert len(funcs) == 1, (cls, name)
    module = ast.Module(body=[ast.ClassDef(name=cls, bases=[], keywords=[], body=funcs, decorator_list=[])], type_ignores=[])
    exec(compile(ast.fix_missing_locations(module), path, "exec"), namespace)
    return namespace[cls]


def cut_functions(root, path, names, namespace):
    tree = ast.parse(open(os.path.join(root, path)).read())
    funcs = [strip(f) for f in tree.body if isinstance(f, ast.FunctionDef) and f.name in names]
    assert sorted(f.name for f in funcs) == sorted(names), [f.name for f in funcs]
    exec(compile(ast.fix_missing_locations(ast.Module(body=funcs, type_ignores=[])), path, "exec"), namespace)


class Bundle:
    """stands in for RayBundle: get_ray_samples records what the sampler hands it"""

    def get_ray_samples(self, **kwargs):
        return types.SimpleNamespace(**kwargs)


def main(root):
    torch.set_default_dtype(torch.float64)
    ns = {"torch": torch, "Tensor": torch.Tensor, "EPS": 1.0e-7}
    pdf_cls = cut_method(root, SAMPLERS, "PDFSampler", "generate_ray_samples", ns)
    cut_functions(root, LOSSES, LOSS_FUNCTIONS, ns)
    n_rays, n_existing, n_new = 8, 12, 9
    edges32, weights32 = ref.make_level(n_rays, n_existing, seed=2025)
    bundle = ref.make_bundle(n_rays, seed=7, dtype=torch.float64)
    nears, fars = bundle.nears, bundle.fars
    s_near, s_far = (ref.SPACING["piecewise"][0](x) for x in (nears, fars))
    fn = lambda x: ref.SPACING["piecewise"][1](x * s_far + (1 - x) * s_near)
    edges, weights = torch.tensor(edges32, dtype=torch.float64), torch.tensor(weights32, dtype=torch.float64)
    existing = types.SimpleNamespace(spacing_starts=edges[..., :-1, None], spacing_ends=edges[..., 1:, None], spacing_to_euclidean_fn=fn)
    arrays = {"edges": edges.numpy(), "weights": weights.numpy(), "nears": nears.numpy(), "fars": fars.numpy()}
    levels = {}
    for tag, training, single, include, padding in (("train_single", True, True, False, 0.01), ("train_each_merged", True, False, True, 0.01),
                                                    ("eval", False, False, False, 1e-5), ("eval_merged", False, False, True, 0.0)):
        sampler = pdf_cls()
        sampler.num_samples, sampler.train_stratified, sampler.training = None, True, training
        sampler.single_jitter, sampler.include_original, sampler.histogram_padding = single, include, padding
        rand = None
        if training:
            torch.manual_seed(11)
            rand = torch.rand((n_rays, 1) if single else (n_rays, n_new + 1))
            torch.manual_seed(11)
        out = sampler.generate_ray_samples(Bundle(), existing, weights, num_samples=n_new)
        bins = torch.cat([out.spacing_starts[..., 0], out.spacing_ends[..., -1:, 0]], -1)
        arrays.update({f"{tag}_rand": rand.numpy() if rand is not None else np.zeros(0), f"{tag}_bins": bins.numpy(),
                       f"{tag}_starts": out.bin_starts.numpy(), f"{tag}_ends": out.bin_ends.numpy()})
        levels[tag] = out
    # the losses: the 12-sample level is the proposal, a pdf level the fine one; the merged level holds every proposal edge (ties)
    for tag in ("train_single", "train_each_merged"):
        fine = levels[tag]
        n_fine = fine.spacing_starts.shape[-2]
        _, w_fine32 = ref.make_level(n_rays, n_fine, seed=31)
        w_fine = torch.tensor(w_fine32, dtype=torch.float64)
        c = ns["ray_samples_to_sdist"](fine)
        arrays.update({f"{tag}_fine_weights": w_fine.numpy(),
                       f"{tag}_outer": ns["outer"](c[..., :-1], c[..., 1:], edges[..., :-1], edges[..., 1:], weights[..., 0]).numpy(),
                       f"{tag}_lossfun_outer": ns["lossfun_outer"](c, w_fine[..., 0], edges, weights[..., 0]).numpy(),
                       f"{tag}_interlevel": ns["interlevel_loss"]([weights, w_fine], [existing, fine]).numpy(),
                       f"{tag}_lossfun_distortion": ns["lossfun_distortion"](c, w_fine[..., 0]).numpy(),
                       f"{tag}_distortion": ns["distortion_loss"]([weights, w_fine], [existing, fine]).numpy()})
    np.savez_compressed(os.path.join(HERE, "ray_sampling.npz"), **arrays)
    print({k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    main(sys.argv[1])
