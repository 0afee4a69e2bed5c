"""Differentiable ray compositing: what lies between a NeRF's per-sample outputs and its loss, over pixie_amd/csrc/ray_render.hip.

The reference's FeatureFieldModel.get_outputs (f3rm/model.py:196-255) turns densities into weights (RaySamples.get_weights,
nerfstudio/cameras/rays.py:129-151) and renders rgb, accumulation, median and expected depth (model_components/renderers.py) and the
C-wide feature (f3rm/renderer.py) from them.  Here that span is one autograd.Function over four kernels:

    get_weights(densities, deltas)                                   (..., S, 1), differentiable in the densities
    composite(densities, deltas, starts, ends, rgb, features, ...)   every output of get_outputs in one call
    RGBRenderer, AccumulationRenderer, DepthRenderer, FeatureRenderer   the reference's classes for unpacked samples: the same kernels
                                                                     with the weights given

Differentiable: densities, rgb, features, and (for the renderers) the weights; `weights` is itself an output of composite that takes
a gradient, which is how the distortion and interlevel losses (pixie_amd.ray_sampling) reach the densities.  Not differentiable: deltas, starts, ends (the
reference detaches the bins), the median depth, and the backward itself.  Deviations from torch's autograd on the same lines
(INTEGRATION 1a row 26): sums run in one fixed order, so results are bit-identical from run to run and under a permutation of the
rays; on a ray with a NaN density the weights from that sample onward are 0 as in the reference, and the gradients, which torch makes
NaN through 0 * NaN, are finite, zero on those samples.  Limits: S <= 1024 (S <= 256 with features), C a multiple of 4 up to 2048,
at most 2^24 rays.  There is no CPU compute path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import RayDesc, RayGrads, RayInputs, RayOutputs, RayUpstream, check

BG_NONE, BG_CONSTANT, BG_LAST_SAMPLE = 0, 1, 2
COLORS = {"black": (0.0, 0.0, 0.0), "white": (1.0, 1.0, 1.0)}


def _background(background):
    """(mode, (r, g, b)) of a reference BackgroundColor: "random" adds nothing, "last_sample", a name, or three host floats"""
    if isinstance(background, str):
        if background == "random":
            return BG_NONE, (0.0, 0.0, 0.0)
        if background == "last_sample":
            return BG_LAST_SAMPLE, (0.0, 0.0, 0.0)
        if background in COLORS:
            return BG_CONSTANT, COLORS[background]
        raise ValueError(f"ray_render: unknown background {background!r}")
    if torch.is_tensor(background):
        if background.device.type != "cpu":
            raise ValueError("ray_render: a constant background is three host floats (a device tensor would need a read-back)")
        background = background.tolist()
    values = tuple(float(v) for v in background)
    if len(values) != 3:
        raise ValueError("ray_render: a constant background has three components")
    return BG_CONSTANT, values


def _require(t, name, shape=None):
    if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"ray_render: {name} must be a contiguous float32 tensor on the device (no CPU path, no conversion)")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"ray_render: {name} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _limits(n_rays, n_samples, n_channels):
    if n_rays < 1 or n_rays > _lib.RAY_MAX_RAYS:
        raise ValueError(f"ray_render: {n_rays} rays, must be in [1, 2^24]")
    if n_samples < 1 or n_samples > _lib.RAY_MAX_SAMPLES:
        raise ValueError(f"ray_render: {n_samples} samples per ray, must be in [1, {_lib.RAY_MAX_SAMPLES}]")
    if n_channels % 4 or n_channels > _lib.RAY_MAX_CHANNELS:
        raise ValueError(f"ray_render: {n_channels} channels, must be a multiple of 4 up to {_lib.RAY_MAX_CHANNELS}")
    if n_channels and n_samples > _lib.RAY_MAX_FEATURE_SAMPLES:
        raise ValueError(f"ray_render: {n_samples} samples per ray with features, at most {_lib.RAY_MAX_FEATURE_SAMPLES}")


def _ptr(t):
    return t.data_ptr() if t is not None else None


class _RayComposite(torch.autograd.Function):
    """args: densities, deltas, weights (given) -- one of densities / weights is None -- starts, ends, rgb, features, all flattened
    to (R, S[, 3 | C]) or None; (mode, bg); want = (accumulation, expected, median, rgb, feature).
    returns (weights or None, accumulation, expected depth (unclipped), median depth, rgb, feature), None where not wanted."""

    @staticmethod
    def forward(ctx, densities, deltas, weights, starts, ends, rgb, features, background, want):
        lead = densities if densities is not None else weights
        n_rays, n_samples = int(lead.shape[0]), int(lead.shape[1])
        n_channels = int(features.shape[-1]) if features is not None else 0
        mode, bg = background
        desc = RayDesc(n_rays, n_samples, n_channels, mode, (C.c_float * 3)(*bg))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=lead.device)
        want_acc, want_exp, want_med, want_rgb, want_feat = want
        out_w = new(n_rays, n_samples) if densities is not None else None
        acc = new(n_rays, 1) if want_acc else None
        exp = new(n_rays, 1) if want_exp else None
        med = new(n_rays, 1) if want_med else None
        out_rgb = new(n_rays, 3) if want_rgb else None
        feat = new(n_rays, n_channels) if want_feat else None
        ins = RayInputs(_ptr(densities), _ptr(deltas), _ptr(weights), _ptr(starts), _ptr(ends), _ptr(rgb), _ptr(features))
        outs = RayOutputs(_ptr(out_w), _ptr(acc), _ptr(exp), _ptr(med), _ptr(out_rgb), _ptr(feat))
        with torch.cuda.device(lead.device):
            check(_lib.load().pixie_ray_composite_forward(C.byref(desc), C.byref(ins), C.byref(outs), _lib.current_stream_ptr()),
                  "pixie_ray_composite_forward")
        ctx.set_materialize_grads(False)
        ctx.shape = (n_rays, n_samples, n_channels, mode, bg)
        ctx.has = tuple(t is not None for t in (densities, deltas, starts, ends, rgb, features))
        ctx.save_for_backward(*[t for t in (densities, deltas, starts, ends, rgb, features) if t is not None],
                              out_w if densities is not None else weights)
        if med is not None:
            ctx.mark_non_differentiable(med)
        return out_w, acc, exp, med, out_rgb, feat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_weights, g_acc, g_exp, g_med, g_rgb, g_feat):
        n_rays, n_samples, n_channels, mode, bg = ctx.shape
        tensors = list(ctx.saved_tensors)
        weights = tensors.pop()
        densities, deltas, starts, ends, rgb, features = [tensors.pop(0) if present else None for present in ctx.has]
        need_density, need_weights, need_rgb, need_feat = (ctx.needs_input_grad[i] for i in (0, 2, 5, 6))
        up = [g.to(torch.float32).contiguous() if g is not None else None for g in (g_weights, g_acc, g_exp, g_rgb, g_feat)]
        if densities is None:
            up[0] = None
        desc = RayDesc(n_rays, n_samples, n_channels, mode, (C.c_float * 3)(*bg))
        d_density = torch.empty_like(densities) if densities is not None and need_density else None
        d_weights = torch.empty_like(weights) if densities is None and need_weights else None
        d_rgb = torch.empty_like(rgb) if rgb is not None and need_rgb and up[3] is not None else None
        d_feat = torch.empty_like(features) if features is not None and need_feat and up[4] is not None else None
        scratch = None
        if up[4] is not None and (d_density is not None or d_weights is not None):
            nbytes = C.c_int64()
            check(_lib.load().pixie_ray_composite_bytes(C.byref(desc), C.byref(nbytes)), "pixie_ray_composite_bytes")
            scratch = torch.empty(max(nbytes.value // 4, 1), dtype=torch.float32, device=weights.device)
        ins = RayInputs(_ptr(densities), _ptr(deltas), _ptr(weights), _ptr(starts), _ptr(ends), _ptr(rgb), _ptr(features))
        ups = RayUpstream(*[_ptr(g) for g in up])
        grads = RayGrads(_ptr(d_density), _ptr(d_weights), _ptr(d_rgb), _ptr(d_feat))
        with torch.cuda.device(weights.device):
            check(_lib.load().pixie_ray_composite_backward(C.byref(desc), C.byref(ins), C.byref(ups), C.byref(grads), _ptr(scratch),
                                                           _lib.current_stream_ptr()), "pixie_ray_composite_backward")
        return d_density, None, d_weights, None, None, d_rgb, d_feat, None, None


def _flatten(t, name, n_last, lead_shape=None):
    """(..., S, n_last) -> (R, S, n_last) (or (R, S) for n_last == 1), checked"""
    _require(t, name)
    if t.dim() < 2 or t.shape[-1] != n_last:
        raise ValueError(f"ray_render: {name} must be (..., S, {n_last}), got {tuple(t.shape)}")
    if lead_shape is not None and tuple(t.shape[:-1]) != tuple(lead_shape):
        raise ValueError(f"ray_render: {name} must be {tuple(lead_shape) + (n_last,)}, got {tuple(t.shape)}")
    n_samples = int(t.shape[-2])
    return t.reshape(-1, n_samples) if n_last == 1 else t.reshape(-1, n_samples, n_last)


def _run(lead_name, lead, deltas, starts, ends, rgb, features, background, want, given_weights):
    """shared front end: checks, flattening of the leading dimensions, one call of the Function, outputs reshaped"""
    flat_lead = _flatten(lead, lead_name, 1)
    batch, lead_shape = tuple(lead.shape[:-2]), tuple(lead.shape[:-1])
    n_channels = 0
    if features is not None:
        _require(features, "features")
        n_channels = int(features.shape[-1])
        if n_channels == 0:
            raise ValueError("ray_render: features must have at least 4 channels")
    _limits(flat_lead.shape[0], flat_lead.shape[1], n_channels)
    flat = lambda t, name, n_last: _flatten(t, name, n_last, lead_shape) if t is not None else None
    args = (flat(deltas, "deltas", 1), flat(starts, "starts", 1), flat(ends, "ends", 1), flat(rgb, "rgb", 3),
            flat(features, "features", n_channels) if features is not None else None)
    for t in args[:3]:
        if t is not None and t.requires_grad:
            raise ValueError("ray_render: deltas, starts and ends get no gradient (the reference detaches the bins); detach them")
    for t in (lead, rgb, features):
        if t is not None and t.device != lead.device:
            raise ValueError("ray_render: all tensors must be on one device")
    mode = _background(background)
    if mode[0] == BG_LAST_SAMPLE and want[3] and rgb is None:
        raise ValueError("ray_render: background last_sample needs rgb")
    if given_weights:
        out = _RayComposite.apply(None, None, flat_lead, args[1], args[2], args[3], args[4], mode, want)
    else:
        out = _RayComposite.apply(flat_lead, args[0], None, args[1], args[2], args[3], args[4], mode, want)
    weights, acc, exp, med, out_rgb, feat = out
    shaped = lambda t, last: t.reshape(batch + (last,)) if t is not None else None
    return (weights.reshape(lead.shape) if weights is not None else None, shaped(acc, 1), shaped(exp, 1), shaped(med, 1), shaped(out_rgb, 3),
            shaped(feat, n_channels))


def _clip_expected(depth, starts, ends):
    """DepthRenderer's clip to [steps.min(), steps.max()], global over the batch: two reductions and a clamp with tensor bounds"""
    steps = (starts + ends) / 2
    return torch.clamp(depth, steps.min(), steps.max())


def get_weights(densities, deltas):
    """RaySamples.get_weights: densities, deltas (..., S, 1) -> weights (..., S, 1)"""
    return _run("densities", densities, deltas, None, None, None, None, "random", (False,) * 5, False)[0]


def composite(densities, deltas, starts, ends, rgb=None, features=None, background="last_sample"):
    """get_weights and every renderer of get_outputs in one call.  densities, deltas, starts, ends (..., S, 1), rgb (..., S, 3),
    features (..., S, C).  Returns dict(weights (..., S, 1), rgb (..., 3) | None, accumulation (..., 1), depth (..., 1) (median, no
    gradient), expected_depth (..., 1), feature (..., C) | None)."""
    weights, acc, exp, med, out_rgb, feat = _run("densities", densities, deltas, starts, ends, rgb, features, background,
                                                 (True, True, True, rgb is not None, features is not None), False)
    return {"weights": weights, "rgb": out_rgb, "accumulation": acc, "depth": med, "expected_depth": _clip_expected(exp, starts, ends),
            "feature": feat}


def _no_packed(ray_indices, num_rays):
    if ray_indices is not None or num_rays is not None:
        raise NotImplementedError("ray_render: packed samples (ray_indices / num_rays) are not supported")


class RGBRenderer(torch.nn.Module):
    """nerfstudio's RGBRenderer for unpacked samples; background_color "random" (nothing added), "last_sample", "black", "white" or
    three host floats"""

    def __init__(self, background_color="random"):
        super().__init__()
        self.background_color = background_color

    @classmethod
    def combine_rgb(cls, rgb, weights, background_color="random", ray_indices=None, num_rays=None):
        _no_packed(ray_indices, num_rays)
        return _run("weights", weights, None, None, None, rgb, None, background_color, (False, False, False, True, False), True)[4]

    def forward(self, rgb, weights, ray_indices=None, num_rays=None, background_color=None):
        if background_color is None:
            background_color = self.background_color
        if not self.training:
            rgb = torch.nan_to_num(rgb)
        out = self.combine_rgb(rgb, weights, background_color=background_color, ray_indices=ray_indices, num_rays=num_rays)
        if not self.training:
            out = torch.clamp(out, min=0.0, max=1.0)
        return out


class AccumulationRenderer(torch.nn.Module):
    @classmethod
    def forward(cls, weights, ray_indices=None, num_rays=None):
        _no_packed(ray_indices, num_rays)
        return _run("weights", weights, None, None, None, None, None, "random", (True, False, False, False, False), True)[1]


class DepthRenderer(torch.nn.Module):
    """method "median" (no gradient) or "expected"; ray_samples is anything with .frustums.starts and .frustums.ends (..., S, 1)"""

    def __init__(self, method="median"):
        super().__init__()
        if method not in ("median", "expected"):
            raise NotImplementedError(f"Method {method} not implemented")
        self.method = method

    def forward(self, weights, ray_samples, ray_indices=None, num_rays=None):
        _no_packed(ray_indices, num_rays)
        starts, ends = ray_samples.frustums.starts, ray_samples.frustums.ends
        if self.method == "median":
            return _run("weights", weights.detach(), None, starts, ends, None, None, "random", (False, False, True, False, False), True)[3]
        depth = _run("weights", weights, None, starts, ends, None, None, "random", (False, True, False, False, False), True)[2]
        return _clip_expected(depth, starts, ends)


class FeatureRenderer(torch.nn.Module):
    """f3rm's FeatureRenderer: sum_i weights_i features_i"""

    @classmethod
    def forward(cls, features, weights):
        if not torch.is_tensor(features) or features.dim() < 2 or features.shape[-1] == 0:
            raise ValueError("ray_render: features must be (..., S, C) with C > 0")
        return _run("weights", weights, None, None, None, None, features, "random", (False, False, False, False, True), True)[5]
