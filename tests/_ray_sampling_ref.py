"""torch restatement of the reference's proposal sampling and its losses, written from those lines and not from the kernels:

    spaced samplers        nerfstudio/model_components/ray_samplers.py:78-248
    pdf sampler            ray_samplers.py:276-372
    proposal sampler       ray_samplers.py:576-617
    get_ray_samples, get_positions    nerfstudio/cameras/rays.py:50-59, 250-294
    outer, lossfun_outer, interlevel_loss, lossfun_distortion, distortion_loss    model_components/losses.py:53-154

Every function runs in the dtype and on the device of its inputs and takes its random numbers as arguments (None: eval mode):
float64 on the CPU is the reference the tests compare with, float32 on the CPU the yardstick whose own distance from float64 sets
the bars, float32 on the device what the benchmark times.  tests/golden/ray_sampling.npz pins these functions to the reference's own
text (tests/golden/make_ray_sampling_golden.py).
"""
import types

import numpy as np
import torch

EPS = 1e-7
KINDS = ("uniform", "lindisp", "sqrt", "log", "piecewise")
SPACING = {
    "uniform": (lambda x: x, lambda x: x),
    "lindisp": (lambda x: 1 / x, lambda x: 1 / x),
    "sqrt": (torch.sqrt, lambda x: x ** 2),
    "log": (torch.log, torch.exp),
    "piecewise": (lambda x: torch.where(x < 1, x / 2, 1 - 1 / (2 * x)), lambda x: torch.where(x < 0.5, 2 * x, 1 / (2 - 2 * x))),
}


def get_ray_samples(bundle, euclidean_bins, bins, fn):
    starts, ends = euclidean_bins[..., :-1, None], euclidean_bins[..., 1:, None]
    frustums = types.SimpleNamespace(origins=bundle.origins[..., None, :], directions=bundle.directions[..., None, :], starts=starts, ends=ends)
    frustums.get_positions = lambda: frustums.origins + frustums.directions * (frustums.starts + frustums.ends) / 2
    return types.SimpleNamespace(frustums=frustums, deltas=ends - starts, spacing_starts=bins[..., :-1, None], spacing_ends=bins[..., 1:, None],
                                 spacing_to_euclidean_fn=fn)


def spaced_bins(num_samples, t_rand, dtype, device):
    """the spacing bins: (1, S + 1) without jitter, (R, S + 1) with t_rand (R, 1) or (R, S + 1)"""
    bins = torch.linspace(0.0, 1.0, num_samples + 1, dtype=dtype).to(device)[None, ...]
    if t_rand is not None:
        bin_centers = (bins[..., 1:] + bins[..., :-1]) / 2.0
        bin_upper = torch.cat([bin_centers, bins[..., -1:]], -1)
        bin_lower = torch.cat([bins[..., :1], bin_centers], -1)
        bins = bin_lower + (bin_upper - bin_lower) * t_rand
    return bins


def spaced_sample(bundle, kind, num_samples, t_rand=None):
    fn, inv = SPACING[kind]
    bins = spaced_bins(num_samples, t_rand, bundle.nears.dtype, bundle.nears.device)
    s_near, s_far = fn(bundle.nears), fn(bundle.fars)

    def spacing_to_euclidean_fn(x):
        return inv(x * s_far + (1 - x) * s_near)

    euclidean_bins = spacing_to_euclidean_fn(bins)
    return get_ray_samples(bundle, euclidean_bins, bins.expand(euclidean_bins.shape), spacing_to_euclidean_fn)


def sdist(ray_samples):
    return torch.cat([ray_samples.spacing_starts[..., 0], ray_samples.spacing_ends[..., -1:, 0]], dim=-1)


def pdf_u(num_samples, batch_shape, rand, dtype, device):
    """the u of the pdf sampler, (*batch_shape, num_samples + 1)"""
    num_bins = num_samples + 1
    u = torch.linspace(0.0, 1.0 - (1.0 / num_bins), steps=num_bins, dtype=dtype, device=device)
    if rand is not None:
        u = u.expand(size=(*batch_shape, num_bins)) + rand / num_bins
    else:
        u = (u + 1.0 / (2 * num_bins)).expand(size=(*batch_shape, num_bins))
    return u.contiguous()


def pdf_cdf(weights, histogram_padding, eps=1e-5):
    """weights (..., S, 1) -> cdf (..., S + 1)"""
    weights = weights[..., 0] + histogram_padding
    weights_sum = torch.sum(weights, dim=-1, keepdim=True)
    padding = torch.relu(eps - weights_sum)
    weights = weights + padding / weights.shape[-1]
    weights_sum = weights_sum + padding
    pdf = weights / weights_sum
    cdf = torch.min(torch.ones_like(pdf), torch.cumsum(pdf, dim=-1))
    return torch.cat([torch.zeros_like(cdf[..., :1]), cdf], dim=-1)


def pdf_bins(existing_bins, weights, num_samples, rand=None, include_original=True, histogram_padding=0.01, eps=1e-5):
    cdf = pdf_cdf(weights, histogram_padding, eps)
    u = pdf_u(num_samples, cdf.shape[:-1], rand, cdf.dtype, cdf.device)
    inds = torch.searchsorted(cdf, u, side="right")
    below = torch.clamp(inds - 1, 0, existing_bins.shape[-1] - 1)
    above = torch.clamp(inds, 0, existing_bins.shape[-1] - 1)
    cdf_g0 = torch.gather(cdf, -1, below)
    bins_g0 = torch.gather(existing_bins, -1, below)
    cdf_g1 = torch.gather(cdf, -1, above)
    bins_g1 = torch.gather(existing_bins, -1, above)
    t = torch.clip(torch.nan_to_num((u - cdf_g0) / (cdf_g1 - cdf_g0), 0), 0, 1)
    bins = bins_g0 + t * (bins_g1 - bins_g0)
    if include_original:
        bins, _ = torch.sort(torch.cat([existing_bins, bins], -1), -1)
    return bins.detach()


def pdf_sample(bundle, ray_samples, weights, num_samples, rand=None, include_original=True, histogram_padding=0.01, eps=1e-5):
    bins = pdf_bins(sdist(ray_samples), weights, num_samples, rand, include_original, histogram_padding, eps)
    return get_ray_samples(bundle, ray_samples.spacing_to_euclidean_fn(bins), bins, ray_samples.spacing_to_euclidean_fn)


def get_weights(ray_samples, densities):
    delta_density = ray_samples.deltas * densities
    alphas = 1 - torch.exp(-delta_density)
    transmittance = torch.cumsum(delta_density[..., :-1, :], dim=-2)
    transmittance = torch.cat([torch.zeros((*transmittance.shape[:1], 1, 1), dtype=densities.dtype, device=densities.device), transmittance], dim=-2)
    return torch.nan_to_num(alphas * torch.exp(-transmittance))


def proposal_sample(bundle, density_fns, proposal_samples, nerf_samples, single_jitter, training, generator_device, anneal=1.0, updated=True,
                    histogram_padding=0.01):
    """ProposalNetworkSampler.generate_ray_samples with the default samplers (piecewise, then pdf without include_original); draws its
    random numbers with torch.rand on generator_device in the reference's order and converts them to the bundle's dtype"""
    n = len(proposal_samples)
    num_rays = bundle.origins.shape[0]
    dtype = bundle.nears.dtype
    weights_list, ray_samples_list = [], []
    weights = ray_samples = None
    for i_level in range(n + 1):
        is_prop = i_level < n
        num_samples = proposal_samples[i_level] if is_prop else nerf_samples
        rand = None
        if training:
            rand = torch.rand((num_rays, 1) if single_jitter else (num_rays, num_samples + 1), dtype=torch.float32, device=generator_device)
            rand = rand.to(device=bundle.nears.device, dtype=dtype)
        if i_level == 0:
            ray_samples = spaced_sample(bundle, "piecewise", num_samples, rand)
        else:
            ray_samples = pdf_sample(bundle, ray_samples, torch.pow(weights, anneal), num_samples, rand, False, histogram_padding)
        if is_prop:
            if updated:
                density = density_fns[i_level](ray_samples.frustums.get_positions())
            else:
                with torch.no_grad():
                    density = density_fns[i_level](ray_samples.frustums.get_positions())
            weights = get_weights(ray_samples, density)
            weights_list.append(weights)
            ray_samples_list.append(ray_samples)
    return ray_samples, weights_list, ray_samples_list


def outer(t0_starts, t0_ends, t1_starts, t1_ends, y1):
    cy1 = torch.cat([torch.zeros_like(y1[..., :1]), torch.cumsum(y1, dim=-1)], dim=-1)
    idx_lo = torch.searchsorted(t1_starts.contiguous(), t0_starts.contiguous(), side="right") - 1
    idx_lo = torch.clamp(idx_lo, min=0, max=y1.shape[-1] - 1)
    idx_hi = torch.searchsorted(t1_ends.contiguous(), t0_ends.contiguous(), side="right")
    idx_hi = torch.clamp(idx_hi, min=0, max=y1.shape[-1] - 1)
    cy1_lo = torch.take_along_dim(cy1[..., :-1], idx_lo, dim=-1)
    cy1_hi = torch.take_along_dim(cy1[..., 1:], idx_hi, dim=-1)
    return cy1_hi - cy1_lo


def lossfun_outer(t, w, t_env, w_env):
    w_outer = outer(t[..., :-1], t[..., 1:], t_env[..., :-1], t_env[..., 1:], w_env)
    return torch.clip(w - w_outer, min=0) ** 2 / (w + EPS)


def interlevel_loss(weights_list, ray_samples_list):
    c = sdist(ray_samples_list[-1]).detach()
    w = weights_list[-1][..., 0].detach()
    loss = 0.0
    for ray_samples, weights in zip(ray_samples_list[:-1], weights_list[:-1]):
        loss = loss + torch.mean(lossfun_outer(c, w, sdist(ray_samples), weights[..., 0]))
    return loss


def lossfun_distortion(t, w):
    ut = (t[..., 1:] + t[..., :-1]) / 2
    dut = torch.abs(ut[..., :, None] - ut[..., None, :])
    loss_inter = torch.sum(w * torch.sum(w[..., None, :] * dut, dim=-1), dim=-1)
    loss_intra = torch.sum(w ** 2 * (t[..., 1:] - t[..., :-1]), dim=-1) / 3
    return loss_inter + loss_intra


def distortion_loss(weights_list, ray_samples_list):
    return torch.mean(lossfun_distortion(sdist(ray_samples_list[-1]), weights_list[-1][..., 0]))


def samples_of_bins(bins):
    """a bare ray_samples that carries spacing bins alone, for the losses"""
    return types.SimpleNamespace(spacing_starts=bins[..., :-1, None], spacing_ends=bins[..., 1:, None])


# ---- the issue's inputs ---------------------------------------------------------------------------------------------------------------
def make_level(n_rays, n_samples, seed=0):
    """S + 1 sorted uniform edges with the ends pinned to 0 and 1, and the get_weights of densities whose optical depth is
    log-uniform in [0.02, 30]; ray 0 has all-zero weights and ray 1 (when there is one) its middle third zero.  float32 arrays."""
    rng = np.random.default_rng(seed)
    edges = np.sort(rng.uniform(0, 1, (n_rays, n_samples + 1)), axis=1)
    edges[:, 0], edges[:, -1] = 0.0, 1.0
    edges = edges.astype(np.float32)
    deltas = np.diff(edges.astype(np.float64), axis=1)
    sigma = np.exp(1.5 * rng.standard_normal((n_rays, n_samples)))
    depth = np.exp(rng.uniform(np.log(0.02), np.log(30.0), (n_rays, 1)))
    x = deltas * sigma
    x = x * depth / np.maximum(x.sum(axis=1, keepdims=True), 1e-30)
    prefix = np.concatenate([np.zeros((n_rays, 1)), np.cumsum(x, axis=1)[:, :-1]], axis=1)
    weights = (1 - np.exp(-x)) * np.exp(-prefix)
    weights[0] = 0.0
    if n_rays > 1:
        weights[1, n_samples // 3: n_samples - n_samples // 3] = 0.0
    return edges, weights.astype(np.float32)[..., None]


def make_bundle(n_rays, seed=0, dtype=torch.float32, device="cpu", near=(0.05, 0.5), far=(2.0, 6.0)):
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n_rays, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    f32 = lambda a: torch.tensor(np.asarray(a, np.float32)).to(device=device, dtype=dtype)
    return types.SimpleNamespace(origins=f32(rng.uniform(-1, 1, (n_rays, 3))), directions=f32(d), nears=f32(rng.uniform(*near, (n_rays, 1))),
                                 fars=f32(rng.uniform(*far, (n_rays, 1))), pixel_area=f32(rng.uniform(1e-6, 1e-5, (n_rays, 1))))


def make_u(n_rays, num_samples, mode, seed=0):
    """the float32 u of a pdf level and the random numbers behind it: mode "single", "per_sample" or "eval" """
    rng = np.random.default_rng(seed)
    rand = None
    if mode == "single":
        rand = torch.tensor(rng.uniform(0, 1, (n_rays, 1)).astype(np.float32))
    elif mode == "per_sample":
        rand = torch.tensor(rng.uniform(0, 1, (n_rays, num_samples + 1)).astype(np.float32))
    return rand, pdf_u(num_samples, (n_rays,), rand, torch.float32, "cpu").numpy()


def step_float32(b, steps):
    b = np.asarray(b, np.float32).copy()
    target = np.float32(np.inf if steps > 0 else -np.inf)
    for _ in range(abs(steps)):
        b = np.nextafter(b, target)
    return b


def pdf_admissible(bins, u, existing_bins, weights, histogram_padding, n_existing, eps=1e-5):
    """the issue's backward-error rule.  F: the float64 restatement's piecewise-linear cdf built from the float32 inputs; b-, b+: b two
    float32 values down / up, clipped to the edge range.  Requires F(b-) - tau <= u <= F(b+) + tau, tau = (S + 16) 2^-24.  Returns
    the worst used share of the allowance: max over the bins of the violation before tau, over tau (<= 1 passes)."""
    tau = (n_existing + 16) * 2.0 ** -24
    edges = np.asarray(existing_bins, np.float32)
    cdf = pdf_cdf(torch.tensor(np.asarray(weights, np.float32), dtype=torch.float64), histogram_padding, eps).numpy()
    worst = 0.0
    for r in range(edges.shape[0]):
        e = edges[r].astype(np.float64)
        down = np.clip(step_float32(bins[r], -2).astype(np.float64), e[0], e[-1])
        up = np.clip(step_float32(bins[r], 2).astype(np.float64), e[0], e[-1])
        f_up, f_down = np.interp(up, e, cdf[r]), np.interp(down, e, cdf[r])
        uu = np.asarray(u[r], np.float64)
        worst = max(worst, float(np.max(f_down - uu)) / tau, float(np.max(uu - f_up)) / tau)
    return worst


def remove_existing(merged, existing):
    """per ray: the merged bins minus one occurrence of every existing edge, compared bit for bit (both rows are sorted); asserts that
    every existing edge is there.  Returns (R, len(merged) - len(existing))."""
    out = []
    for m, e in zip(np.asarray(merged, np.float32), np.asarray(existing, np.float32)):
        mb, eb = m.view(np.uint32), e.view(np.uint32)
        keep, j = [], 0
        for i in range(len(m)):
            if j < len(e) and mb[i] == eb[j]:
                j += 1
            else:
                keep.append(m[i])
        assert j == len(e), "an existing edge is missing from the merged bins"
        out.append(keep)
    return np.asarray(out, np.float32)


# (rays, existing samples, requested samples, histogram_padding, u mode, include_original): the pdf sampler's cases, shared by the CPU
# check of the admissibility rule on the float32 restatement and the device test
PDF_CASES = (
    (1, 1, 1, 0.01, "eval", False), (3, 2, 3, 1e-5, "single", False), (130, 63, 48, 0.0, "per_sample", False),
    (130, 64, 49, 0.01, "single", True), (3, 65, 96, 1e-5, "eval", False), (130, 256, 96, 0.01, "single", False),
    (3, 256, 257, 0.0, "per_sample", True), (3, 1024, 1023, 1e-5, "single", False), (130, 1024, 48, 0.01, "eval", False),
    (3, 1, 1023, 0.0, "per_sample", False), (130, 2, 257, 0.01, "per_sample", False), (3, 63, 1, 1e-5, "eval", True),
    (130, 65, 3, 0.0, "single", True), (1, 256, 48, 1e-5, "per_sample", False), (3, 64, 96, 0.0, "eval", False),
    (130, 96, 48, 0.01, "single", False), (3, 1024, 1, 0.0, "eval", False), (130, 63, 1023, 1e-5, "single", False),
    (3, 2, 49, 0.01, "eval", True), (130, 65, 257, 1e-5, "per_sample", False), (3, 256, 3, 0.0, "single", False),
)


def pdf_case_inputs(case, index):
    n_rays, n_existing, n_new, padding, mode, include = case
    edges, weights = make_level(n_rays, n_existing, seed=100 + index)
    rand, u = make_u(n_rays, n_new, mode, seed=200 + index)
    return edges, weights, rand, u
