#!/usr/bin/env python
"""Times one training pass (forward + backward) of the ray compositing tail of FeatureFieldModel.get_outputs through
pixie_amd.ray_render against the reference's lines as torch ops under autograd, and writes a table (default
profiles/ray_composite_table.txt); recorded, not asserted.

Shape: R = 4096 rays x S = 48 samples, rgb and C = 768 feature channels (f3rm_config.py:35), background last_sample; and the two
weights-only proposal levels, S = 256 and S = 96 (get_weights forward + backward alone).  Inputs as in tests/_ray_render_ref.py:
sorted edges, log-normal densities with a log-uniform optical depth per ray, uniform rgb, normal features; the upstream gradients of
weights, rgb, accumulation, expected depth and feature are fixed standard-normal arrays, all at once.
  * composite: ray_render.composite + backward: two launches forward (ray, feature), two backward (feature, ray), the clip's three torch ops.
  * split: get_weights + RGBRenderer, DepthRenderer (median under no_grad, expected), AccumulationRenderer, FeatureRenderer + backward:
    the reference's call sequence on the same kernels.
  * torch: the reference's lines (rays.py:139-151, renderers.py:103-118, 315, 353-382, f3rm/renderer.py:15) as torch ops, autograd.
  * feature forward alone: FeatureRenderer under no_grad, one launch; feature pass: FeatureRenderer + backward with the weights and the
    features requiring gradients (feature forward, feature backward, ray backward); the backward kernel's time is not separated.
Traffic floor of the feature sum: B = 4 R S C bytes read once forward, read once and written once backward: 3 B per pass.  The table
gives 3 B / (composite time) in TB/s -- the whole pass, ray kernels and torch ops included, charged to the feature traffic -- and
B / (feature forward alone).
Method: the candidates alternate in the same process after `--warmup` rounds; each sample is HIP events around one pass; the table
gives the median over `--reps` samples and the spread.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from field_query_bench import DEV, alternate  # noqa: E402
from pixie_amd import ray_render  # noqa: E402


def make_inputs(gen, n_rays, n_samples, n_channels):
    rand = lambda *s: torch.rand(s, generator=gen, device=DEV)
    randn = lambda *s: torch.randn(s, generator=gen, device=DEV)
    edges = torch.sort(rand(n_rays, n_samples + 1) * 4 + 0.05, dim=1).values
    starts, ends = edges[:, :-1, None].contiguous(), edges[:, 1:, None].contiguous()
    deltas = ends - starts
    sigma = torch.exp(1.5 * randn(n_rays, n_samples, 1))
    depth = torch.exp(rand(n_rays, 1, 1) * (torch.log(torch.tensor(30.0)) - torch.log(torch.tensor(0.02))) + torch.log(torch.tensor(0.02)))
    sigma = (sigma * depth / (deltas * sigma).sum(dim=1, keepdim=True)).contiguous()
    t = SimpleNamespace(densities=sigma.requires_grad_(True), deltas=deltas, starts=starts, ends=ends,
                        rgb=rand(n_rays, n_samples, 3).requires_grad_(True),
                        features=randn(n_rays, n_samples, n_channels).requires_grad_(True) if n_channels else None)
    t.up = {"weights": randn(n_rays, n_samples, 1), "rgb": randn(n_rays, 3), "accumulation": randn(n_rays, 1), "expected_depth": randn(n_rays, 1),
            "feature": randn(n_rays, n_channels) if n_channels else None}
    t.samples = SimpleNamespace(frustums=SimpleNamespace(starts=starts, ends=ends))
    return t


def backward(t, out):
    for leaf in (t.densities, t.rgb, t.features):
        if leaf is not None:
            leaf.grad = None
    keys = [k for k in t.up if t.up[k] is not None and out.get(k) is not None]
    torch.autograd.backward([out[k] for k in keys], [t.up[k] for k in keys])


def composite_pass(t):
    backward(t, ray_render.composite(t.densities, t.deltas, t.starts, t.ends, t.rgb, t.features, "last_sample"))


RENDERERS = SimpleNamespace(rgb=ray_render.RGBRenderer("last_sample"), median=ray_render.DepthRenderer("median"),
                            expected=ray_render.DepthRenderer("expected"), accumulation=ray_render.AccumulationRenderer(),
                            feature=ray_render.FeatureRenderer())


def split_pass(t):
    weights = ray_render.get_weights(t.densities, t.deltas)
    out = {"weights": weights, "rgb": RENDERERS.rgb(rgb=t.rgb, weights=weights)}
    with torch.no_grad():
        RENDERERS.median(weights=weights, ray_samples=t.samples)
    out["expected_depth"] = RENDERERS.expected(weights=weights, ray_samples=t.samples)
    out["accumulation"] = RENDERERS.accumulation(weights=weights)
    out["feature"] = RENDERERS.feature(features=t.features, weights=weights)
    backward(t, out)


def torch_weights(densities, deltas):
    delta_density = deltas * densities
    alphas = 1 - torch.exp(-delta_density)
    transmittance = torch.cumsum(delta_density[..., :-1, :], dim=-2)
    transmittance = torch.cat([torch.zeros((*transmittance.shape[:1], 1, 1), device=densities.device), transmittance], dim=-2)
    transmittance = torch.exp(-transmittance)
    return torch.nan_to_num(alphas * transmittance)


def torch_pass(t):
    weights = torch_weights(t.densities, t.deltas)
    comp_rgb = torch.sum(weights * t.rgb, dim=-2)
    accumulated_weight = torch.sum(weights, dim=-2)
    out = {"weights": weights, "rgb": comp_rgb + t.rgb[..., -1, :] * (1.0 - accumulated_weight)}
    steps = (t.starts + t.ends) / 2
    with torch.no_grad():
        cumulative_weights = torch.cumsum(weights[..., 0], dim=-1)
        split = torch.ones((*weights.shape[:-2], 1), device=weights.device) * 0.5
        median_index = torch.clamp(torch.searchsorted(cumulative_weights, split, side="left"), 0, steps.shape[-2] - 1)
        torch.gather(steps[..., 0], dim=-1, index=median_index)
    depth = torch.sum(weights * steps, dim=-2) / (torch.sum(weights, -2) + 1e-10)
    out["expected_depth"] = torch.clip(depth, steps.min(), steps.max())
    out["accumulation"] = torch.sum(weights, dim=-2)
    out["feature"] = torch.sum(weights * t.features, dim=-2)
    backward(t, out)


def weights_pass(fn, t):
    t.densities.grad = None
    fn(t.densities, t.deltas).backward(t.up["weights"])


def feature_forward_alone(t, weights):
    with torch.no_grad():
        RENDERERS.feature(features=t.features, weights=weights)


def feature_pass(t, weights):
    weights.grad, t.features.grad = None, None
    RENDERERS.feature(features=t.features, weights=weights).backward(t.up["feature"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=48)
    ap.add_argument("--channels", type=int, default=768)
    ap.add_argument("--levels", type=int, nargs="*", default=[256, 96])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the achieved rate is divided by")
    ap.add_argument("--no-torch", action="store_true", help="leave the torch baseline out (for a kernel trace of the kernels alone)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ray_composite_table.txt"))
    args = ap.parse_args()
    gen = torch.Generator(device=DEV).manual_seed(0)
    cell = lambda v: f"{v[0]:8.3f} ({v[1]:.3f} .. {v[2]:.3f})"
    R, S, Cn = args.rays, args.samples, args.channels
    t = make_inputs(gen, R, S, Cn)
    given = ray_render.get_weights(t.densities, t.deltas).detach().requires_grad_(True)
    cands = {"composite": lambda: composite_pass(t), "split": lambda: split_pass(t), "torch": lambda: torch_pass(t),
             "feature forward alone": lambda: feature_forward_alone(t, given), "feature pass": lambda: feature_pass(t, given)}
    if args.no_torch:
        del cands["torch"]
    times = alternate(cands, args.warmup, args.reps)
    B = 4.0 * R * S * Cn
    lines = [f"ray compositing training pass (forward + backward), {torch.cuda.get_device_name(0)}; ms, median (min .. max) of {args.reps} samples",
             f"R = {R}, S = {S}, C = {Cn}, rgb, background last_sample; feature array B = {B / 1e6:.0f} MB"]
    for name, v in times.items():
        row = f"{name:>24} {cell(v):>30}"
        if name == "torch":
            row += f"   torch / composite {v[0] / times['composite'][0]:6.2f}"
        if name in ("composite", "split", "feature pass"):
            rate = 3 * B / 1e12 / (v[0] / 1e3)
            row += f"   3 B / time {rate:5.2f} TB/s = {rate / args.peak_tbs:4.2f} of {args.peak_tbs:g} TB/s"
        if name == "feature forward alone":
            rate = B / 1e12 / (v[0] / 1e3)
            row += f"   B / time   {rate:5.2f} TB/s = {rate / args.peak_tbs:4.2f} of {args.peak_tbs:g} TB/s"
        lines.append(row)
    for S_level in args.levels:
        lv = make_inputs(gen, R, S_level, 0)
        cands = {"get_weights": lambda lv=lv: weights_pass(ray_render.get_weights, lv), "torch": lambda lv=lv: weights_pass(torch_weights, lv)}
        if args.no_torch:
            del cands["torch"]
        v = alternate(cands, args.warmup, args.reps)
        row = f"weights only, R = {R}, S = {S_level}: get_weights forward + backward {cell(v['get_weights'])}"
        if "torch" in v:
            row += f", torch {cell(v['torch'])}, torch / ours {v['torch'][0] / v['get_weights'][0]:.2f}"
        lines.append(row)
    lines.append("3 B / time charges the whole pass (ray kernels, allocations and the clip's torch ops included) to the feature traffic floor of one read forward,")
    lines.append("one read and one write backward; the two feature kernels are not timed apart from each other (feature pass = forward + backward + ray backward).")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
