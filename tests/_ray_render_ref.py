"""torch restatement of the reference's ray compositing lines, written from those lines and not from the kernels:

    get_weights            nerfstudio/cameras/rays.py:129-151
    combine_rgb            nerfstudio/model_components/renderers.py:103-118 (unpacked branch)
    accumulation           renderers.py:315
    median / expected      renderers.py:353-382
    feature                f3rm/renderer.py:15

Every function runs in the dtype of its inputs: float64 on the CPU is the reference the tests compare with, float32 on the CPU the
yardstick whose own distance from float64 sets the bar.  Gradients come from autograd.  tests/golden/ray_composite.npz pins these
functions to the reference's own text (tests/golden/make_ray_composite_golden.py).
"""
import numpy as np
import torch

COLORS = {"black": (0.0, 0.0, 0.0), "white": (1.0, 1.0, 1.0)}
OUTPUTS = ("weights", "rgb", "accumulation", "expected_depth", "feature")


def get_weights(densities, deltas):
    delta_density = deltas * densities
    alphas = 1 - torch.exp(-delta_density)
    transmittance = torch.cumsum(delta_density[..., :-1, :], dim=-2)
    transmittance = torch.cat([torch.zeros((*transmittance.shape[:-2], 1, 1), dtype=densities.dtype), transmittance], dim=-2)
    transmittance = torch.exp(-transmittance)
    weights = alphas * transmittance
    return torch.nan_to_num(weights)


def combine_rgb(rgb, weights, background="random"):
    comp_rgb = torch.sum(weights * rgb, dim=-2)
    accumulated_weight = torch.sum(weights, dim=-2)
    if isinstance(background, str) and background == "random":
        return comp_rgb
    if isinstance(background, str) and background == "last_sample":
        bg = rgb[..., -1, :]
    else:
        bg = torch.tensor(COLORS[background] if isinstance(background, str) else [float(v) for v in background], dtype=rgb.dtype).expand(comp_rgb.shape)
    return comp_rgb + bg * (1.0 - accumulated_weight)


def accumulation(weights):
    return torch.sum(weights, dim=-2)


def steps_of(starts, ends):
    return (starts + ends) / 2


def median_depth(weights, starts, ends):
    steps = steps_of(starts, ends)
    cumulative_weights = torch.cumsum(weights[..., 0], dim=-1)
    split = torch.ones((*weights.shape[:-2], 1), dtype=weights.dtype) * 0.5
    median_index = torch.searchsorted(cumulative_weights, split, side="left")
    median_index = torch.clamp(median_index, 0, steps.shape[-2] - 1)
    return torch.gather(steps[..., 0], dim=-1, index=median_index)


def expected_depth(weights, starts, ends, clip=True):
    eps = 1e-10
    steps = steps_of(starts, ends)
    depth = torch.sum(weights * steps, dim=-2) / (torch.sum(weights, -2) + eps)
    return torch.clip(depth, steps.min(), steps.max()) if clip else depth


def feature(features, weights):
    return torch.sum(weights * features, dim=-2)


def get_outputs(densities, deltas, starts, ends, rgb=None, features=None, background="last_sample", keep=None):
    """the tail of FeatureFieldModel.get_outputs.  keep (..., S, 1) of 0 / 1 multiplies the weights: the documented masking of a ray
    with a NaN density, evaluated on densities from which the NaN has been removed."""
    weights = get_weights(densities, deltas)
    if keep is not None:
        weights = weights * keep
    out = {"weights": weights, "accumulation": accumulation(weights), "expected_depth": expected_depth(weights, starts, ends)}
    with torch.no_grad():
        out["depth"] = median_depth(weights, starts, ends)
    out["rgb"] = combine_rgb(rgb, weights, background) if rgb is not None else None
    out["feature"] = feature(features, weights) if features is not None else None
    return out


def evaluate(inputs, upstream, dtype, background="last_sample", keep=None):
    """inputs: dict of numpy arrays (densities, deltas, starts, ends, rgb | None, features | None); upstream: dict of numpy arrays for
    OUTPUTS (None where absent).  Returns (outputs, grads) as dicts of float64 numpy arrays; grads of densities, rgb, features for
    loss = sum over outputs of <output, upstream>."""
    t = {k: (torch.tensor(np.asarray(v), dtype=dtype) if v is not None else None) for k, v in inputs.items()}
    for k in ("densities", "rgb", "features"):
        if t.get(k) is not None:
            t[k].requires_grad_(True)
    out = get_outputs(t["densities"], t["deltas"], t["starts"], t["ends"], t.get("rgb"), t.get("features"), background,
                      torch.tensor(keep, dtype=dtype) if keep is not None else None)
    loss = None
    for k in OUTPUTS:
        if out.get(k) is not None and upstream.get(k) is not None:
            term = (out[k] * torch.tensor(upstream[k], dtype=dtype)).sum()
            loss = term if loss is None else loss + term
    grads = {}
    if loss is not None:
        loss.backward()
        grads = {k: t[k].grad.double().numpy() for k in ("densities", "rgb", "features") if t.get(k) is not None and t[k].grad is not None}
    return {k: (v.detach().double().numpy() if v is not None else None) for k, v in out.items()}, grads


def make_inputs(n_rays, n_samples, n_channels, seed=0, rgb=True):
    """the issue's inputs: S + 1 sorted edges in [0.05, 4.05]; densities exp(1.5 N(0, 1)) rescaled so that the ray's optical depth
    sum delta sigma is log-uniform in [0.02, 30]; rgb uniform; features standard normal.  float32 numpy arrays."""
    rng = np.random.default_rng(seed)
    edges = np.sort(rng.uniform(0.05, 4.05, (n_rays, n_samples + 1)), axis=1).astype(np.float32)
    starts, ends = edges[:, :-1, None].copy(), edges[:, 1:, None].copy()
    deltas = (ends - starts).astype(np.float32)
    sigma = np.exp(1.5 * rng.standard_normal((n_rays, n_samples, 1)))
    depth = np.exp(rng.uniform(np.log(0.02), np.log(30.0), (n_rays, 1, 1)))
    sigma = sigma * depth / np.maximum((deltas.astype(np.float64) * sigma).sum(axis=1, keepdims=True), 1e-30)
    out = {"densities": sigma.astype(np.float32), "deltas": deltas, "starts": starts, "ends": ends,
           "rgb": rng.uniform(0, 1, (n_rays, n_samples, 3)).astype(np.float32) if rgb else None,
           "features": rng.standard_normal((n_rays, n_samples, n_channels)).astype(np.float32) if n_channels else None}
    return out


def make_upstream(n_rays, n_samples, n_channels, seed=1, rgb=True):
    """fixed random upstream gradients for every output at once"""
    rng = np.random.default_rng(seed)
    g = lambda *s: rng.standard_normal(s).astype(np.float32)
    return {"weights": g(n_rays, n_samples, 1), "rgb": g(n_rays, 3) if rgb else None, "accumulation": g(n_rays, 1), "expected_depth": g(n_rays, 1),
            "feature": g(n_rays, n_channels) if n_channels else None}


def bar(ref64, yard32, terms):
    """_field_query_ref.bar's form: 3 x the float32 yardstick's own distance from float64, plus (terms + 16) 2^-24 max(1, max |ref|),
    terms = the number of terms of the longest sum behind the array"""
    ref64 = np.asarray(ref64, np.float64)
    scale = max(1.0, float(np.max(np.abs(ref64)))) if ref64.size else 1.0
    return 3.0 * float(np.max(np.abs(np.asarray(yard32, np.float64) - ref64), initial=0.0)) + (terms + 16) * 2.0 ** -24 * scale


def median_admissible(got32, weights64, starts32, ends32, n_samples):
    """per ray: is the returned median depth bit-equal to the float32 mid-point of an index j with cum64[j] >= 0.5 - tau and
    (j == 0 or cum64[j - 1] < 0.5 + tau), tau = S 2^-23; a ray that never reaches 0.5 + tau may also return the last sample"""
    tau = n_samples * 2.0 ** -23
    cum = np.cumsum(np.asarray(weights64, np.float64)[..., 0], axis=-1)
    mid = ((starts32[..., 0].astype(np.float32) + ends32[..., 0].astype(np.float32)) / np.float32(2)).astype(np.float32)
    ok = cum >= 0.5 - tau
    ok[:, 1:] &= cum[:, :-1] < 0.5 + tau
    ok[:, -1] |= cum[:, -1] < 0.5 + tau          # never reached: the clamp to S - 1
    if n_samples > 1:
        ok[:, -1] &= cum[:, -2] < 0.5 + tau
    hit = (mid.view(np.uint32) == np.asarray(got32, np.float32).reshape(-1, 1).view(np.uint32)) & ok
    return hit.any(axis=1)
