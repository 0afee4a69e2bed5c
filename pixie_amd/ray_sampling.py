"""Proposal sampling and the two losses that exist because of it, over pixie_amd/csrc/ray_sample.hip.

The first line of the reference's FeatureFieldModel.get_outputs (f3rm/model.py:199) is ProposalNetworkSampler -> UniformLinDispPiecewiseSampler
/ UniformSampler -> PDFSampler (nerfstudio/model_components/ray_samplers.py:53-372, 522-617); interlevel_loss and distortion_loss
(model_components/losses.py:54-154) read what it returns.  Here

    UniformSampler, LinearDisparitySampler, SqrtSampler, LogSampler, UniformLinDispPiecewiseSampler    one kernel, one launch
    PDFSampler                                  one launch for the whole of generate_ray_samples, annealing included
    ProposalNetworkSampler                      the reference's loop over the caller's density_fns
    interlevel_loss, lossfun_outer              differentiable in the proposal weights
    distortion_loss, lossfun_distortion         differentiable in the weights; no (R, S, S) array

Both samplers also return Frustums.get_positions() from the same launch.  Random numbers are drawn here with torch.rand, in the
reference's shapes and order, and the linspace tables come from torch.linspace (cached), so a seeded run consumes the generator as the
reference does.  The samplers have no gradient (the reference detaches the bins); the losses have no double backward.  Deviations from
torch on the same lines: sums run in one fixed order, so results are bit-identical from run to run and under a
permutation of the rays; the annealing power is float(pow(double)); a ray with a NaN weight gets all its new bins on its last existing
edge.  Limits: at most 1024 existing and 1024 produced samples per ray (include_original counts), 2^24 rays, 8 proposal levels.  A ray
bundle is anything with .origins, .directions (R, 3), .nears, .fars (R, 1) and optionally .pixel_area.  There is no CPU compute path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ray_render
from ._lib import (RayDistortionDesc, RayInterlevelDesc, RayInterlevelGrads, RayInterlevelInputs, RaySampleDesc, RaySampleInputs,
                   RaySampleOutputs, check)

SPACING_FOREIGN, SPACING_UNIFORM, SPACING_LINDISP, SPACING_SQRT, SPACING_LOG, SPACING_PIECEWISE = -1, 0, 1, 2, 3, 4
MAX_SAMPLES, MAX_RAYS, MAX_LEVELS = _lib.RAY_SAMPLE_MAX_SAMPLES, _lib.RAY_MAX_RAYS, _lib.RAY_SAMPLE_MAX_LEVELS

_SPACING_FN = {
    SPACING_UNIFORM: (lambda x: x, lambda x: x),
    SPACING_LINDISP: (lambda x: 1 / x, lambda x: 1 / x),
    SPACING_SQRT: (torch.sqrt, lambda x: x ** 2),
    SPACING_LOG: (torch.log, torch.exp),
    SPACING_PIECEWISE: (lambda x: torch.where(x < 1, x / 2, 1 - 1 / (2 * x)), lambda x: torch.where(x < 0.5, 2 * x, 1 / (2 - 2 * x))),
}


def _require(t, name, shape=None):
    if not torch.is_tensor(t) or t.device.type != "cuda" or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"ray_sampling: {name} must be a contiguous float32 tensor on the device (no CPU path, no conversion)")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"ray_sampling: {name} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _limits(n_rays, n_samples, what="samples per ray"):
    if n_rays < 1 or n_rays > MAX_RAYS:
        raise ValueError(f"ray_sampling: {n_rays} rays, must be in [1, 2^24]")
    if n_samples < 1 or n_samples > MAX_SAMPLES:
        raise ValueError(f"ray_sampling: {n_samples} {what}, must be in [1, {MAX_SAMPLES}]")


def _ptr(t):
    return t.data_ptr() if t is not None else None


_tables = {}


def _linspace_table(kind, steps, device):
    """the reference's torch.linspace tables, from torch's own op, cached per (steps, device): "spaced" is computed on the CPU and
    copied, "pdf" is computed on the device, each as the reference does"""
    key = (kind, steps, str(device))
    if key not in _tables:
        if kind == "spaced":
            _tables[key] = torch.linspace(0.0, 1.0, steps).to(device)
        else:
            _tables[key] = torch.linspace(0.0, 1.0 - (1.0 / steps), steps=steps, device=device)
    return _tables[key]


class SpacingToEuclidean:
    """spacing_to_euclidean_fn of a spaced sampler: callable on a (R, K) tensor in torch, and carrying (kind, s_near, s_far) so that
    PDFSampler applies it in-kernel.  s_near, s_far: (R, 1)."""

    def __init__(self, kind, s_near, s_far):
        self.kind, self.s_near, self.s_far = kind, s_near, s_far

    def __call__(self, x):
        return _SPACING_FN[self.kind][1](x * self.s_far + (1 - x) * self.s_near)


class Frustums:
    """origins, directions (R, 1, 3), starts, ends (R, S, 1), pixel_area (R, 1, 1) or None"""

    def __init__(self, origins, directions, starts, ends, pixel_area=None, positions=None):
        self.origins, self.directions, self.starts, self.ends, self.pixel_area = origins, directions, starts, ends, pixel_area
        self.offsets = None
        self._positions = positions

    def get_positions(self):
        pos = self._positions
        if pos is None:
            pos = self.origins + self.directions * (self.starts + self.ends) / 2
        if self.offsets is not None:
            pos = pos + self.offsets
        return pos

    def set_offsets(self, offsets):
        self.offsets = offsets


class RaySamples:
    """what ray_render.DepthRenderer, the density_fns and the losses read.  spacing_bins (R, S + 1) is the kernel's own output;
    spacing_starts / spacing_ends (R, S, 1) are views of it."""

    def __init__(self, frustums, deltas, spacing_bins, spacing_to_euclidean_fn):
        self.frustums, self.deltas, self.spacing_bins, self.spacing_to_euclidean_fn = frustums, deltas, spacing_bins, spacing_to_euclidean_fn
        self.spacing_starts, self.spacing_ends = spacing_bins[..., :-1, None], spacing_bins[..., 1:, None]

    def get_weights(self, densities):
        return ray_render.get_weights(densities, self.deltas)


def _bundle(ray_bundle):
    if ray_bundle is None or getattr(ray_bundle, "nears", None) is None or getattr(ray_bundle, "fars", None) is None:
        raise ValueError("ray_sampling: a ray bundle with nears and fars is required")
    origins = _require(ray_bundle.origins, "origins")
    if origins.dim() != 2 or origins.shape[1] != 3:
        raise ValueError(f"ray_sampling: origins must be (R, 3), got {tuple(origins.shape)}")
    n_rays = int(origins.shape[0])
    _require(ray_bundle.directions, "directions", (n_rays, 3))
    _require(ray_bundle.nears, "nears", (n_rays, 1))
    _require(ray_bundle.fars, "fars", (n_rays, 1))
    return n_rays


def _samples_of(ray_bundle, n_rays, n_out, spacing_fn, want_positions, launch):
    """allocates the outputs, runs `launch(outs)` and wraps them"""
    device = ray_bundle.origins.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
    foreign = not isinstance(spacing_fn, SpacingToEuclidean)
    bins = new(n_rays, n_out + 1)
    if foreign:
        starts = ends = deltas = positions = None
    else:
        starts, ends, deltas = new(n_rays, n_out, 1), new(n_rays, n_out, 1), new(n_rays, n_out, 1)
        positions = new(n_rays, n_out, 3) if want_positions else None
    launch(bins, starts, ends, deltas, positions)
    if foreign:
        euclidean = spacing_fn(bins)
        starts, ends = euclidean[..., :-1, None].contiguous(), euclidean[..., 1:, None].contiguous()
        deltas = ends - starts
    pixel_area = getattr(ray_bundle, "pixel_area", None)
    frustums = Frustums(ray_bundle.origins[:, None, :], ray_bundle.directions[:, None, :], starts, ends,
                        pixel_area[:, None, :] if pixel_area is not None else None, positions)
    return RaySamples(frustums, deltas, bins, spacing_fn)


class Sampler(torch.nn.Module):
    def __init__(self, num_samples=None):
        super().__init__()
        self.num_samples = num_samples

    def forward(self, *args, **kwargs):
        return self.generate_ray_samples(*args, **kwargs)


class SpacedSampler(Sampler):
    """spacing: one of the SPACING_* kinds (the reference passes a pair of callables; the kinds are its five subclasses)"""

    def __init__(self, spacing, num_samples=None, train_stratified=True, single_jitter=False, positions=True):
        super().__init__(num_samples=num_samples)
        if spacing not in _SPACING_FN:
            raise ValueError(f"ray_sampling: unknown spacing kind {spacing!r}")
        self.spacing, self.train_stratified, self.single_jitter, self.positions = spacing, train_stratified, single_jitter, positions

    def generate_ray_samples(self, ray_bundle=None, num_samples=None):
        n_rays = _bundle(ray_bundle)
        num_samples = num_samples or self.num_samples
        if num_samples is None:
            raise ValueError("ray_sampling: num_samples is not set")
        _limits(n_rays, num_samples)
        device = ray_bundle.origins.device
        table = _linspace_table("spaced", num_samples + 1, device)
        jitter = None
        if self.train_stratified and self.training:
            jitter = torch.rand((n_rays, 1) if self.single_jitter else (n_rays, num_samples + 1), dtype=torch.float32, device=device)
        s_near, s_far = torch.empty_like(ray_bundle.nears), torch.empty_like(ray_bundle.fars)
        desc = RaySampleDesc(n_rays, num_samples, 0, self.spacing, int(jitter.shape[1]) if jitter is not None else 0, 0, 0.0, 0.0, 1.0, 0.0, 0.0)

        def launch(bins, starts, ends, deltas, positions):
            ins = RaySampleInputs(_ptr(ray_bundle.nears), _ptr(ray_bundle.fars), _ptr(ray_bundle.origins), _ptr(ray_bundle.directions),
                                  _ptr(table), _ptr(jitter), None, None, None, None)
            outs = RaySampleOutputs(_ptr(bins), _ptr(starts), _ptr(ends), _ptr(deltas), _ptr(positions), _ptr(s_near), _ptr(s_far))
            with torch.cuda.device(device):
                check(_lib.load().pixie_ray_sample_spaced(C.byref(desc), C.byref(ins), C.byref(outs), _lib.current_stream_ptr()),
                      "pixie_ray_sample_spaced")

        return _samples_of(ray_bundle, n_rays, num_samples, SpacingToEuclidean(self.spacing, s_near, s_far), self.positions, launch)


def _spaced(kind):
    class _Kind(SpacedSampler):
        def __init__(self, num_samples=None, train_stratified=True, single_jitter=False, positions=True):
            super().__init__(kind, num_samples=num_samples, train_stratified=train_stratified, single_jitter=single_jitter, positions=positions)
    return _Kind


UniformSampler = _spaced(SPACING_UNIFORM)
LinearDisparitySampler = _spaced(SPACING_LINDISP)
SqrtSampler = _spaced(SPACING_SQRT)
LogSampler = _spaced(SPACING_LOG)
UniformLinDispPiecewiseSampler = _spaced(SPACING_PIECEWISE)
for _name in ("UniformSampler", "LinearDisparitySampler", "SqrtSampler", "LogSampler", "UniformLinDispPiecewiseSampler"):
    globals()[_name].__name__ = globals()[_name].__qualname__ = _name


def _existing_bins(ray_samples):
    bins = getattr(ray_samples, "spacing_bins", None)
    if bins is None:
        if ray_samples.spacing_starts is None or ray_samples.spacing_ends is None:
            raise ValueError("ray_sampling: ray_samples need spacing_starts and spacing_ends")
        bins = torch.cat([ray_samples.spacing_starts[..., 0], ray_samples.spacing_ends[..., -1:, 0]], dim=-1)
    return bins.detach().contiguous()


class PDFSampler(Sampler):
    def __init__(self, num_samples=None, train_stratified=True, single_jitter=False, include_original=True, histogram_padding=0.01,
                 positions=True):
        super().__init__(num_samples=num_samples)
        self.train_stratified, self.single_jitter, self.include_original = train_stratified, single_jitter, include_original
        self.histogram_padding, self.positions = histogram_padding, positions

    def generate_ray_samples(self, ray_bundle=None, ray_samples=None, weights=None, num_samples=None, eps=1e-5, anneal=1.0):
        """anneal: ProposalNetworkSampler's exponent, applied to the weights in the kernel (1 skips it)"""
        if ray_samples is None or ray_bundle is None:
            raise ValueError("ray_samples and ray_bundle must be provided")
        if weights is None:
            raise ValueError("ray_sampling: weights must be provided")
        n_rays = _bundle(ray_bundle)
        num_samples = num_samples or self.num_samples
        if num_samples is None:
            raise ValueError("ray_sampling: num_samples is not set")
        if ray_samples.spacing_to_euclidean_fn is None:
            raise ValueError("ray_sampling: ray_samples.spacing_to_euclidean_fn must be provided")
        existing = _existing_bins(ray_samples)
        if not torch.is_tensor(weights) or weights.dim() != 3 or weights.shape[-1] != 1:
            raise ValueError("ray_sampling: weights must be (R, S, 1)")
        n_existing = int(weights.shape[1])
        _limits(n_rays, num_samples)
        _limits(n_rays, n_existing, "existing samples per ray")
        n_out = num_samples + n_existing + 1 if self.include_original else num_samples
        _limits(n_rays, n_out, "samples per ray with include_original")
        weights = _require(weights.detach(), "weights", (n_rays, n_existing, 1))
        _require(existing, "the existing spacing bins", (n_rays, n_existing + 1))
        device = ray_bundle.origins.device
        num_bins = num_samples + 1
        table = _linspace_table("pdf", num_bins, device)
        jitter = None
        if self.train_stratified and self.training:
            jitter = torch.rand((n_rays, 1) if self.single_jitter else (n_rays, num_samples + 1), device=device)
        fn = ray_samples.spacing_to_euclidean_fn
        ours = isinstance(fn, SpacingToEuclidean)
        u_scale = float(np.float32(1.0) / np.float32(num_bins))    # torch on the device: rand / num_bins is rand * float32(1 / num_bins)
        u_offset = float(np.float32(1.0 / (2 * num_bins)))
        desc = RaySampleDesc(n_rays, num_samples, n_existing, fn.kind if ours else SPACING_FOREIGN, int(jitter.shape[1]) if jitter is not None else 0,
                             int(bool(self.include_original)), float(self.histogram_padding), float(eps), float(anneal), u_scale, u_offset)

        def launch(bins, starts, ends, deltas, positions):
            ins = RaySampleInputs(None, None, _ptr(ray_bundle.origins), _ptr(ray_bundle.directions), _ptr(table), _ptr(jitter), _ptr(existing),
                                  _ptr(weights), _ptr(fn.s_near) if ours else None, _ptr(fn.s_far) if ours else None)
            outs = RaySampleOutputs(_ptr(bins), _ptr(starts), _ptr(ends), _ptr(deltas), _ptr(positions), None, None)
            with torch.cuda.device(device):
                check(_lib.load().pixie_ray_sample_pdf(C.byref(desc), C.byref(ins), C.byref(outs), _lib.current_stream_ptr()),
                      "pixie_ray_sample_pdf")

        return _samples_of(ray_bundle, n_rays, n_out, fn, self.positions, launch)


class ProposalNetworkSampler(Sampler):
    """the reference's ProposalNetworkSampler; density_fns are the caller's (positions (R, S, 3) -> densities (R, S, 1))"""

    def __init__(self, num_proposal_samples_per_ray=(64,), num_nerf_samples_per_ray=32, num_proposal_network_iterations=2, single_jitter=False,
                 update_sched=lambda x: 1, initial_sampler=None, pdf_sampler=None):
        super().__init__()
        self.num_proposal_samples_per_ray = num_proposal_samples_per_ray
        self.num_nerf_samples_per_ray = num_nerf_samples_per_ray
        self.num_proposal_network_iterations = num_proposal_network_iterations
        self.update_sched = update_sched
        if self.num_proposal_network_iterations < 1:
            raise ValueError("num_proposal_network_iterations must be >= 1")
        self.initial_sampler = UniformLinDispPiecewiseSampler(single_jitter=single_jitter) if initial_sampler is None else initial_sampler
        self.pdf_sampler = PDFSampler(include_original=False, single_jitter=single_jitter) if pdf_sampler is None else pdf_sampler
        self._anneal = 1.0
        self._steps_since_update = 0
        self._step = 0

    def set_anneal(self, anneal):
        self._anneal = anneal

    def step_cb(self, step):
        self._step = step
        self._steps_since_update += 1

    def generate_ray_samples(self, ray_bundle=None, density_fns=None):
        if ray_bundle is None or density_fns is None:
            raise ValueError("ray_sampling: ray_bundle and density_fns are required")
        weights_list, ray_samples_list = [], []
        n = self.num_proposal_network_iterations
        weights = ray_samples = None
        updated = self._steps_since_update > self.update_sched(self._step) or self._step < 10
        for i_level in range(n + 1):
            is_prop = i_level < n
            num_samples = self.num_proposal_samples_per_ray[i_level] if is_prop else self.num_nerf_samples_per_ray
            if i_level == 0:
                ray_samples = self.initial_sampler(ray_bundle, num_samples=num_samples)
            elif isinstance(self.pdf_sampler, PDFSampler):
                ray_samples = self.pdf_sampler(ray_bundle, ray_samples, weights, num_samples=num_samples, anneal=self._anneal)
            else:
                ray_samples = self.pdf_sampler(ray_bundle, ray_samples, torch.pow(weights, self._anneal), num_samples=num_samples)
            if is_prop:
                if updated:
                    density = density_fns[i_level](ray_samples.frustums.get_positions())
                else:
                    with torch.no_grad():
                        density = density_fns[i_level](ray_samples.frustums.get_positions())
                weights = ray_samples.get_weights(density)
                weights_list.append(weights)
                ray_samples_list.append(ray_samples)
        if updated:
            self._steps_since_update = 0
        return ray_samples, weights_list, ray_samples_list


# ---- losses ---------------------------------------------------------------------------------------------------------------------------
def _edges_weights(t, w, what):
    """(R, S + 1) edges and (R, S) weights, checked; the weights keep their autograd history"""
    _require(t, what + " edges")
    if t.dim() != 2 or t.shape[1] < 2:
        raise ValueError(f"ray_sampling: {what} edges must be (R, S + 1), got {tuple(t.shape)}")
    n_rays, n_samples = int(t.shape[0]), int(t.shape[1]) - 1
    _limits(n_rays, n_samples)
    _require(w, what + " weights", (n_rays, n_samples))
    if t.requires_grad:
        raise ValueError("ray_sampling: edges get no gradient (the reference detaches the bins); detach them")
    return n_rays, n_samples


def _upstream(g):
    return g.to(torch.float32).contiguous()


class _Interlevel(torch.autograd.Function):
    """args: c (R, S + 1), w (R, S), per_sample, then (edges, weights) per proposal level.  Returns the scalar loss, or with
    per_sample the (R, S) terms of the one level."""

    @staticmethod
    def forward(ctx, c, w, per_sample, *levels):
        edges, weights = levels[0::2], levels[1::2]
        n_rays, n_fine = int(w.shape[0]), int(w.shape[1])
        sizes = [int(x.shape[1]) for x in weights]
        pad = [0] * (MAX_LEVELS - len(sizes))
        desc = RayInterlevelDesc(n_rays, n_fine, len(sizes), (C.c_int32 * MAX_LEVELS)(*(sizes + pad)), int(per_sample))
        none = [None] * len(pad)
        ins = RayInterlevelInputs(_ptr(c), _ptr(w), (C.c_void_p * MAX_LEVELS)(*([_ptr(e) for e in edges] + none)),
                                  (C.c_void_p * MAX_LEVELS)(*([_ptr(x) for x in weights] + none)))
        lib = _lib.load()
        with torch.cuda.device(w.device):
            if per_sample:
                out = torch.empty_like(w)
                check(lib.pixie_ray_interlevel_forward(C.byref(desc), C.byref(ins), None, _ptr(out), None, _lib.current_stream_ptr()),
                      "pixie_ray_interlevel_forward")
            else:
                nbytes = C.c_int64()
                check(lib.pixie_ray_interlevel_bytes(C.byref(desc), C.byref(nbytes)), "pixie_ray_interlevel_bytes")
                scratch = torch.empty(nbytes.value // 4, dtype=torch.float32, device=w.device)
                out = torch.empty((), dtype=torch.float32, device=w.device)
                check(lib.pixie_ray_interlevel_forward(C.byref(desc), C.byref(ins), _ptr(out), None, _ptr(scratch), _lib.current_stream_ptr()),
                      "pixie_ray_interlevel_forward")
        ctx.desc, ctx.ins = desc, ins
        ctx.save_for_backward(c, w, *levels)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved = ctx.saved_tensors
        weights = saved[3::2]
        need = ctx.needs_input_grad[4::2]
        grads = [torch.empty_like(x) if n else None for x, n in zip(weights, need)]
        out = (C.c_void_p * MAX_LEVELS)(*([_ptr(x) for x in grads] + [None] * (MAX_LEVELS - len(grads))))
        g = _upstream(g)
        with torch.cuda.device(g.device):
            check(_lib.load().pixie_ray_interlevel_backward(C.byref(ctx.desc), C.byref(ctx.ins), _ptr(g), C.byref(RayInterlevelGrads(out)),
                                                            _lib.current_stream_ptr()), "pixie_ray_interlevel_backward")
        result = [None, None, None]
        for x in grads:
            result += [None, x]
        return tuple(result)


class _Distortion(torch.autograd.Function):
    """t (R, S + 1), w (R, S) -> the mean over the rays, or with per_ray lossfun_distortion's (R) values"""

    @staticmethod
    def forward(ctx, t, w, per_ray):
        n_rays, n_samples = int(w.shape[0]), int(w.shape[1])
        desc = RayDistortionDesc(n_rays, n_samples, int(per_ray))
        values = torch.empty(n_rays, dtype=torch.float32, device=w.device)
        out = None if per_ray else torch.empty((), dtype=torch.float32, device=w.device)
        with torch.cuda.device(w.device):
            check(_lib.load().pixie_ray_distortion_forward(C.byref(desc), _ptr(t), _ptr(w), _ptr(out), _ptr(values), _lib.current_stream_ptr()),
                  "pixie_ray_distortion_forward")
        ctx.desc = desc
        ctx.save_for_backward(t, w)
        return values if per_ray else out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        t, w = ctx.saved_tensors
        if not ctx.needs_input_grad[1]:
            return None, None, None
        g = _upstream(g)
        grad = torch.empty_like(w)
        with torch.cuda.device(w.device):
            check(_lib.load().pixie_ray_distortion_backward(C.byref(ctx.desc), _ptr(t), _ptr(w), _ptr(g), _ptr(grad), _lib.current_stream_ptr()),
                  "pixie_ray_distortion_backward")
        return None, grad, None


def lossfun_outer(t, w, t_env, w_env):
    """losses.lossfun_outer: t (R, S + 1), w (R, S), t_env (R, S_env + 1), w_env (R, S_env) -> (R, S); differentiable in w_env alone"""
    n_rays, _ = _edges_weights(t, w, "fine")
    if _edges_weights(t_env, w_env, "proposal")[0] != n_rays:
        raise ValueError("ray_sampling: the two levels must have the same rays")
    if w.requires_grad:
        raise ValueError("ray_sampling: the enveloped weights get no gradient here (interlevel_loss detaches them); detach them")
    return _Interlevel.apply(t, w, True, t_env, w_env)


def ray_samples_to_sdist(ray_samples):
    return _existing_bins(ray_samples)


def _level_weights(weights):
    if not torch.is_tensor(weights) or weights.dim() != 3 or weights.shape[-1] != 1:
        raise ValueError("ray_sampling: weights must be (R, S, 1)")
    return weights[..., 0]


def interlevel_loss(weights_list, ray_samples_list):
    """losses.interlevel_loss: the last level's (detached) histogram against every level before it"""
    if len(ray_samples_list) < 2 or len(weights_list) != len(ray_samples_list):
        raise ValueError("ray_sampling: interlevel_loss needs at least one proposal level and the fine level")
    if len(weights_list) - 1 > MAX_LEVELS:
        raise ValueError(f"ray_sampling: {len(weights_list) - 1} proposal levels, at most {MAX_LEVELS}")
    c = ray_samples_to_sdist(ray_samples_list[-1])
    w = _level_weights(weights_list[-1]).detach()
    n_rays, _ = _edges_weights(c, w, "fine")
    levels = []
    for ray_samples, weights in zip(ray_samples_list[:-1], weights_list[:-1]):
        cp, wp = ray_samples_to_sdist(ray_samples), _level_weights(weights)
        if _edges_weights(cp, wp, "proposal")[0] != n_rays:
            raise ValueError("ray_sampling: all levels must have the same rays")
        levels += [cp, wp]
    return _Interlevel.apply(c, w, False, *levels)


def lossfun_distortion(t, w):
    """losses.lossfun_distortion: t (R, S + 1), w (R, S) -> (R)"""
    _edges_weights(t, w, "the")
    return _Distortion.apply(t, w, True)


def distortion_loss(weights_list, ray_samples_list):
    """losses.distortion_loss: the mean of lossfun_distortion over the last level's rays"""
    c = ray_samples_to_sdist(ray_samples_list[-1])
    w = _level_weights(weights_list[-1])
    _edges_weights(c, w, "the")
    return _Distortion.apply(c, w, False)
