#!/usr/bin/env python
"""Writes tests/golden/gs_densify.npz: GaussianModel.densify_and_prune computed by the REFERENCE's own
gaussian-splatting/scene/gaussian_model.py, loaded unmodified from its path and run on CPU torch, for
tests/test_gs_optim_ref.py and tests/test_gs_densify_hip.py.

How the unmodified module runs without a device: `simple_knn._C` and `plyfile` are stub modules (neither is used on this route);
torch.zeros / ones / empty / tensor / full drop a device="cuda" argument; torch.cuda.empty_cache is a no-op; torch.normal is
replaced by mean + std * z for the recorded z, so the split's draw is an input of the golden.

Per case of tests/_gs_optim_ref.py's GOLDEN_CASES:
  <case>.before.*   the float32 state densify_and_prune starts from: the six parameters and their moments after ONE
                    optimizer.step() of the reference's Adam on random gradients (so the moments are non-zero), the statistics
  <case>.z          the (2 n_split, 3) standard-normal draw the split consumed
  <case>.after32.*  the reference's result at float32: parameters, moments, statistics, and the optimiser's `step`
  <case>.after64.*  the float64 twin (the same float32 state cast up, default dtype float64): parameters only
Build container only (needs the reference tree); only data is committed.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/third_party/PhysGaussian/gaussian-splatting"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _gs_optim_ref as gr  # noqa: E402

GROUP_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
              "rotation": "_rotation"}


def load_reference():
    knn = types.ModuleType("simple_knn")
    knn_c = types.ModuleType("simple_knn._C")
    knn_c.distCUDA2 = None
    knn._C = knn_c
    ply = types.ModuleType("plyfile")
    ply.PlyData = ply.PlyElement = None
    sys.modules.update({"simple_knn": knn, "simple_knn._C": knn_c, "plyfile": ply})
    for fn in ("zeros", "ones", "empty", "tensor", "full"):
        real = getattr(torch, fn)

        def on_host(*a, _real=real, **kw):
            if str(kw.get("device", "")).startswith("cuda"):
                kw.pop("device")
            return _real(*a, **kw)
        setattr(torch, fn, on_host)
    torch.cuda.empty_cache = lambda: None
    sys.path.insert(0, REF)
    from scene.gaussian_model import GaussianModel
    return GaussianModel


def training_args():
    return argparse.Namespace(percent_dense=gr.PERCENT_DENSE, position_lr_init=1.6e-4, position_lr_final=1.6e-6, position_lr_delay_mult=0.01,
                              position_lr_max_steps=30000, feature_lr=2.5e-3, opacity_lr=5e-4, scaling_lr=5e-5, rotation_lr=1e-3)


def model_from(GaussianModel, degree, arrays, dtype):
    m = GaussianModel(degree)
    m.spatial_lr_scale = 1.0
    for f, attr in GROUP_ATTR.items():
        setattr(m, attr, torch.nn.Parameter(torch.from_numpy(arrays[f]).to(dtype).requires_grad_(True)))
    m.training_setup(training_args())
    return m


def state_of(m):
    out = {}
    for group in m.optimizer.param_groups:
        p = group["params"][0]
        out[group["name"]] = p.detach().numpy().copy()
        st = m.optimizer.state[p]
        out["exp_avg." + group["name"]] = st["exp_avg"].numpy().copy()
        out["exp_avg_sq." + group["name"]] = st["exp_avg_sq"].numpy().copy()
        out["step." + group["name"]] = np.float64(float(st["step"]))
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        out[k] = getattr(m, k).numpy().copy()
    return out


def main():
    GaussianModel = load_reference()
    real_normal = torch.normal
    out = {"cases": np.array(list(gr.GOLDEN_CASES))}
    for name, (n, degree, mss, _) in gr.GOLDEN_CASES.items():
        case = gr.make_case(name)
        rng = np.random.default_rng(n + 17)
        # float32: one step of the reference's optimiser, so that the moments densify_and_prune carries over are non-zero
        m = model_from(GaussianModel, degree, case, torch.float32)
        for group in m.optimizer.param_groups:
            p = group["params"][0]
            p.grad = torch.from_numpy((rng.normal(0, 1, p.shape) * 10.0 ** rng.uniform(-6, 0, p.shape)).astype(np.float32))
        m.optimizer.step()
        for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            setattr(m, k, torch.from_numpy(case[k].copy()))
        before = state_of(m)
        for k, v in before.items():
            out[f"{name}.before.{k}"] = v
        assert min(gr.margins(before).values()) > 1e-3, gr.margins(before)
        used = {}

        def normal(mean, std, _z=case["z"], _used=used):
            z = torch.from_numpy(_z[:std.shape[0]]).to(std.dtype)
            _used["z"] = _z[:std.shape[0]].copy()
            return mean + std * z
        torch.normal = normal
        m.densify_and_prune(gr.MAX_GRAD, gr.MIN_OPACITY, gr.EXTENT, mss)
        out[f"{name}.z"] = used["z"]
        for k, v in state_of(m).items():
            out[f"{name}.after32.{k}"] = v

        # the float64 twin: the same float32 state, cast up
        torch.set_default_dtype(torch.float64)
        m64 = model_from(GaussianModel, degree, before, torch.float64)
        for group in m64.optimizer.param_groups:
            f = group["name"]
            m64.optimizer.state[group["params"][0]] = {"step": torch.tensor(1.0), "exp_avg": torch.from_numpy(before["exp_avg." + f]).double(),
                                                       "exp_avg_sq": torch.from_numpy(before["exp_avg_sq." + f]).double()}
        for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            setattr(m64, k, torch.from_numpy(before[k]).double())
        m64.densify_and_prune(gr.MAX_GRAD, gr.MIN_OPACITY, gr.EXTENT, mss)
        torch.set_default_dtype(torch.float32)
        torch.normal = real_normal
        after64 = state_of(m64)
        for f in gr.FIELDS:
            out[f"{name}.after64.{f}"] = after64[f]
        print(name, "rows", n, "->", after64["xyz"].shape[0], "split", used["z"].shape[0] // 2 if "z" in used else 0)
    path = os.path.join(HERE, "gs_densify.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
