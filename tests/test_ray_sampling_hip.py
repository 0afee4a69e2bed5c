"""GPU checks of proposal sampling and its losses (pixie_amd.ray_sampling, pixie_amd/csrc/ray_sample.hip) against the torch restatement
of the reference's lines in tests/_ray_sampling_ref.py.

PDF bins: a backward-error rule, not a forward difference (at padding 1e-5 the float32 restatement itself sits 2e-4 from float64: the
inverse cdf has slope width / pdf).  F is the float64 restatement's piecewise-linear cdf of the float32 inputs; b-, b+ are b two float32
values down / up, clipped to the edge range; F(b-) - tau <= u <= F(b+) + tau, tau = (S + 16) 2^-24.  Each ray's bins are non-decreasing;
with include_original every existing edge is present bit for bit.  tests/test_ray_sampling_math.py holds the float32 restatement to
half that allowance on the same inputs.

Everything downstream of the bins is compared with float32 NumPy evaluated from the bins the kernel returned: bit-equal for uniform,
lindisp and piecewise, within 2 ulp for sqrt and log.

Losses, value and gradient: max |got - ref64| <= 3 x max |yard32 - ref64| + (terms + 16) 2^-24 max(1, max |ref64|), ref64 the float64
autograd of the restatement on the same float32 inputs, yard32 the restatement in float32 on the CPU; terms = S_env for interlevel,
S for the distortion gradient, S^2 for the distortion value (the double sum is direct).  The upstream scalar is R S (interlevel) or R
(distortion), so that the gradients are O(1) under that bar.

The measured ratios are appended to the file named by PIXIE_RAY_SAMPLING_PARITY_OUT when it is set (profiles/ray_sampling_parity.txt
is such a run's output).
"""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import _ray_render_ref as rref
from tests import _ray_sampling_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
KIND = {"uniform": 0, "lindisp": 1, "sqrt": 2, "log": 3, "piecewise": 4}
ONE, TWO, HALF = F32(1), F32(2), F32(0.5)
NP_FN = {"uniform": (lambda v: v, lambda v: v), "lindisp": (lambda v: ONE / v, lambda v: ONE / v),
         "piecewise": (lambda v: np.where(v < ONE, v / TWO, ONE - ONE / (TWO * v)), lambda v: np.where(v < HALF, TWO * v, ONE / (TWO - TWO * v))),
         "sqrt": (np.sqrt, lambda v: v * v), "log": (np.log, np.exp)}


def note(line):
    print(line)
    path = os.environ.get("PIXIE_RAY_SAMPLING_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def ulps(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return int(np.max(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)), initial=0))


def fixed_rand(monkeypatch, values):
    """torch.rand returns `values` (None: must not be called): the sampler then runs on the random numbers of the CPU check"""
    def rand(*args, **kwargs):
        assert values is not None, "eval mode draws no random numbers"
        shape = tuple(args[0]) if len(args) == 1 and not isinstance(args[0], int) else tuple(args)
        assert shape == tuple(values.shape), (shape, values.shape)
        return values.to(DEV)
    monkeypatch.setattr(torch, "rand", rand)


def device_bundle(n_rays, seed=0, **kw):
    b = ref.make_bundle(n_rays, seed=seed, **kw)
    return types.SimpleNamespace(**{k: v.to(DEV) for k, v in vars(b).items()})


def existing_samples(edges, kind, bundle):
    """our RaySamples around given spacing bins: what a previous level would have handed to the pdf sampler"""
    from pixie_amd import ray_sampling as rs
    s_near, s_far = (ref.SPACING[kind][0](x) for x in (bundle.nears, bundle.fars))
    return rs.RaySamples(None, None, dev(edges), rs.SpacingToEuclidean(KIND[kind], s_near.contiguous(), s_far.contiguous()))


def check_downstream(samples, kind, bundle, what):
    """euclidean starts / ends from the returned spacing bins, deltas and positions from the returned starts / ends, in float32 NumPy"""
    fn = samples.spacing_to_euclidean_fn
    bins, s_near, s_far = host(samples.spacing_bins), host(fn.s_near), host(fn.s_far)
    with np.errstate(all="ignore"):
        euclidean = NP_FN[kind][1]((bins * s_far + (ONE - bins) * s_near).astype(F32)).astype(F32)
    starts, ends = host(samples.frustums.starts), host(samples.frustums.ends)
    assert starts.shape == ends.shape == (bins.shape[0], bins.shape[1] - 1, 1) and samples.deltas.shape == starts.shape
    if kind in ("sqrt", "log"):
        assert ulps(starts[..., 0], euclidean[:, :-1]) <= 2 and ulps(ends[..., 0], euclidean[:, 1:]) <= 2, what
    else:
        assert bits_equal(starts[..., 0], euclidean[:, :-1]) and bits_equal(ends[..., 0], euclidean[:, 1:]), what
    assert bits_equal(host(samples.deltas), ends - starts), what
    o, d = host(bundle.origins)[:, None, :], host(bundle.directions)[:, None, :]
    assert bits_equal(host(samples.frustums.get_positions()), o + d * (starts + ends) / TWO), what
    assert torch.equal(samples.spacing_starts[..., 0], samples.spacing_bins[:, :-1]) and torch.equal(samples.spacing_ends[..., 0], samples.spacing_bins[:, 1:])
    assert samples.frustums.origins.shape == (bins.shape[0], 1, 3) and samples.frustums.pixel_area.shape == (bins.shape[0], 1, 1)


# ---- 5 / 6. the pdf sampler ------------------------------------------------------------------------------------------------------------
def run_pdf(monkeypatch, case, index, kind, order=None):
    from pixie_amd import ray_sampling as rs
    n_rays, n_existing, n_new, padding, mode, include = case
    edges, weights, rand, u = ref.pdf_case_inputs(case, index)
    bundle = device_bundle(n_rays, seed=index)
    if order is not None:
        edges, weights, u = edges[order], weights[order], u[order]
        rand = rand[order] if rand is not None else None
        bundle = types.SimpleNamespace(**{k: v[torch.as_tensor(order, device=DEV)].contiguous() for k, v in vars(bundle).items()})
    fixed_rand(monkeypatch, rand)
    sampler = rs.PDFSampler(num_samples=n_new, single_jitter=mode == "single", include_original=include, histogram_padding=padding)
    sampler.train(mode != "eval")
    out = sampler(bundle, existing_samples(edges, kind, bundle), dev(weights))
    return out, bundle, edges, weights, u


@pytest.mark.parametrize("index", range(len(ref.PDF_CASES)))
def test_pdf_sampler_bins_are_admissible_and_the_rest_follows(monkeypatch, index):
    case = ref.PDF_CASES[index]
    n_rays, n_existing, n_new, padding, mode, include = case
    kind = ref.KINDS[index % 5]
    out, bundle, edges, weights, u = run_pdf(monkeypatch, case, index, kind)
    bins = host(out.spacing_bins)
    assert bins.shape == (n_rays, (n_new + n_existing + 2) if include else n_new + 1) and np.all(np.isfinite(bins))
    assert np.all(np.diff(bins, axis=1) >= 0), case
    fresh = ref.remove_existing(bins, edges) if include else bins
    worst = ref.pdf_admissible(fresh, u, edges, weights, padding, n_existing)
    note(f"pdf R={n_rays} S={n_existing} N={n_new} padding={padding:g} u={mode} include_original={include} kind={kind}: "
         f"share of the allowance used {worst:.3f}")
    assert worst <= 1.0, (case, worst)
    check_downstream(out, kind, bundle, case)


def test_pdf_sampler_annealing_and_foreign_spacing(monkeypatch):
    from pixie_amd import ray_sampling as rs
    case, index = (130, 64, 49, 0.01, "single", False), 40
    edges, weights, rand, u = ref.pdf_case_inputs(case, index)
    bundle = device_bundle(130, seed=index)
    fixed_rand(monkeypatch, rand)
    sampler = rs.PDFSampler(num_samples=49, single_jitter=True, include_original=False)
    existing = existing_samples(edges, "piecewise", bundle)
    annealed = sampler(bundle, existing, dev(weights), anneal=0.5)
    powered = (weights.astype(np.float64) ** 0.5).astype(F32)
    worst = ref.pdf_admissible(host(annealed.spacing_bins), u, edges, powered, 0.01, 64)
    note(f"pdf anneal=0.5 R=130 S=64 N=49: share of the allowance used {worst:.3f}")
    assert worst <= 1.0
    plain = sampler(bundle, existing, dev(weights))
    fn = existing.spacing_to_euclidean_fn
    existing.spacing_to_euclidean_fn = lambda x: fn(x)             # a foreign callable: applied in torch to the kernel's bins
    existing.spacing_bins = None                                   # and foreign samples carry starts and ends alone
    foreign = sampler(bundle, existing, dev(weights))
    assert torch.equal(foreign.spacing_bins, plain.spacing_bins)
    assert torch.equal(foreign.frustums.starts, plain.frustums.starts) and torch.equal(foreign.deltas, plain.deltas)
    assert torch.equal(foreign.frustums.get_positions(), plain.frustums.get_positions())


# ---- 6. the spaced samplers ------------------------------------------------------------------------------------------------------------
SPACED_SHAPES = ((1, 1), (3, 2), (130, 63), (3, 64), (130, 65), (3, 256), (3, 1024), (130, 48), (3, 96), (130, 257), (1, 1023), (3, 3), (130, 49),
                 (3, 1023), (130, 256))


@pytest.mark.parametrize("index", range(15))
def test_spaced_samplers(monkeypatch, index):
    from pixie_amd import ray_sampling as rs
    kind, mode = ref.KINDS[index % 5], ("single", "per_sample", "eval")[index // 5]
    n_rays, n_samples = SPACED_SHAPES[index]
    bundle = device_bundle(n_rays, seed=index, near=(0.05, 2.0), far=(2.5, 6.0))      # nears on both sides of 1
    rng = np.random.default_rng(index)
    rand = None if mode == "eval" else torch.tensor(rng.uniform(0, 1, (n_rays, 1 if mode == "single" else n_samples + 1)).astype(F32))
    fixed_rand(monkeypatch, rand)
    cls = {"uniform": rs.UniformSampler, "lindisp": rs.LinearDisparitySampler, "sqrt": rs.SqrtSampler, "log": rs.LogSampler,
           "piecewise": rs.UniformLinDispPiecewiseSampler}[kind]
    sampler = cls(num_samples=n_samples, single_jitter=mode == "single")
    sampler.train(mode != "eval")
    out = sampler(bundle)
    want = ref.spaced_bins(n_samples, rand, torch.float32, "cpu").expand(n_rays, n_samples + 1).numpy()
    assert bits_equal(host(out.spacing_bins), want), (kind, mode)
    fn = out.spacing_to_euclidean_fn
    with np.errstate(all="ignore"):
        s_near, s_far = NP_FN[kind][0](host(bundle.nears)).astype(F32), NP_FN[kind][0](host(bundle.fars)).astype(F32)
    if kind in ("sqrt", "log"):
        assert ulps(host(fn.s_near), s_near) <= 2 and ulps(host(fn.s_far), s_far) <= 2
    else:
        assert bits_equal(host(fn.s_near), s_near) and bits_equal(host(fn.s_far), s_far)
    check_downstream(out, kind, bundle, (kind, mode))
    if kind == "piecewise":
        assert (host(bundle.nears) < 1).any() and (host(bundle.nears) > 1).any()


# ---- 7. the losses ---------------------------------------------------------------------------------------------------------------------
def within(what, got, r64, r32, terms):
    got, r64 = np.asarray(got, np.float64), np.asarray(r64, np.float64)
    assert got.shape == r64.shape and np.all(np.isfinite(got)), what
    err = float(np.max(np.abs(got - r64), initial=0.0))
    bar = rref.bar(r64, r32, terms)
    yard = float(np.max(np.abs(np.asarray(r32, np.float64) - r64), initial=0.0))
    note(f"{what}: error {err:.3e}, float32 restatement {yard:.3e}, bar {bar:.3e}, ratio {err / bar:.3f}")
    assert err <= bar, (what, err, bar)


def tied_fine_edges(edges, weights, n_new, index):
    """a fine level made by our pdf sampler with include_original=True from the proposal level: every proposal edge occurs in it"""
    from pixie_amd import ray_sampling as rs
    bundle = device_bundle(edges.shape[0], seed=index)
    sampler = rs.PDFSampler(num_samples=n_new, include_original=True).eval()
    return host(sampler(bundle, existing_samples(edges, "uniform", bundle), dev(weights)).spacing_bins)


# (rays, proposal level sizes, fine samples, tie case)
INTERLEVEL_CASES = ((1, (1,), 1, False), (3, (12,), 9, False), (130, (256, 96), 48, False), (3, (1024,), 257, False), (3, (2, 63), 1023, False),
                    (130, (64,), 114, True), (3, (65, 256, 49), 96, False))


@functools.lru_cache(maxsize=None)
def interlevel_reference(index):
    """inputs and the restatement's value and gradients in float64 and float32: computed once, shared, never modified"""
    n_rays, sizes, n_fine, ties = INTERLEVEL_CASES[index]
    levels = [ref.make_level(n_rays, s, seed=300 + 10 * index + k) for k, s in enumerate(sizes)]
    c, w = ref.make_level(n_rays, n_fine, seed=400 + index)
    if ties:
        c = tied_fine_edges(levels[-1][0], levels[-1][1], n_fine - sizes[-1] - 1, index)
    scale = float(n_rays * n_fine)

    def evaluate(dtype):
        t = lambda a: torch.tensor(a, dtype=dtype)
        ws = [t(lw).requires_grad_(True) for _, lw in levels]
        loss = ref.interlevel_loss(ws + [t(w)], [ref.samples_of_bins(t(e)) for e, _ in levels] + [ref.samples_of_bins(t(c))])
        (loss * scale).backward()
        return loss.detach().double().numpy(), [x.grad.double().numpy() for x in ws]

    return levels, c, w, scale, evaluate(torch.float64), evaluate(torch.float32)


def ours_interlevel(levels, c, w, scale, order=None):
    from pixie_amd import ray_sampling as rs
    pick = (lambda a: a) if order is None else (lambda a: a[order])
    ws = [dev(pick(lw)).requires_grad_(True) for _, lw in levels]
    samples = [ref.samples_of_bins(dev(pick(e))) for e, _ in levels] + [ref.samples_of_bins(dev(pick(c)))]
    loss = rs.interlevel_loss(ws + [dev(pick(w))], samples)
    (loss * scale).backward()
    return host(loss), [host(x.grad) for x in ws]


@pytest.mark.parametrize("index", range(len(INTERLEVEL_CASES)))
def test_interlevel_loss_value_and_gradient(index):
    n_rays, sizes, n_fine, ties = INTERLEVEL_CASES[index]
    levels, c, w, scale, (v64, g64), (v32, g32) = interlevel_reference(index)
    assert c.shape == (n_rays, n_fine + 1)
    if ties:
        ref.remove_existing(c, levels[-1][0])                      # asserts that every proposal edge is a fine edge
    value, grads = ours_interlevel(levels, c, w, scale)
    what = f"interlevel R={n_rays} levels={sizes} S={n_fine} ties={ties}"
    within(what + " value", value, v64, v32, max(sizes))
    for k, s in enumerate(sizes):
        assert np.any(g64[k] != 0) or n_fine == 1
        within(what + f" d_weights[{k}]", grads[k], g64[k], g32[k], s)


DISTORTION_CASES = ((1, 1), (3, 2), (130, 48), (130, 63), (3, 64), (130, 65), (3, 256), (3, 1024))


@functools.lru_cache(maxsize=None)
def distortion_reference(index):
    n_rays, n_samples = DISTORTION_CASES[index]
    t_np, w_np = ref.make_level(n_rays, n_samples, seed=500 + index)
    scale = float(n_rays)

    def evaluate(dtype):
        w = torch.tensor(w_np, dtype=dtype).requires_grad_(True)
        loss = ref.distortion_loss([w], [ref.samples_of_bins(torch.tensor(t_np, dtype=dtype))])
        (loss * scale).backward()
        return loss.detach().double().numpy(), w.grad.double().numpy()

    return t_np, w_np, scale, evaluate(torch.float64), evaluate(torch.float32)


def ours_distortion(t_np, w_np, scale, order=None):
    from pixie_amd import ray_sampling as rs
    pick = (lambda a: a) if order is None else (lambda a: a[order])
    w = dev(pick(w_np)).requires_grad_(True)
    loss = rs.distortion_loss([w], [ref.samples_of_bins(dev(pick(t_np)))])
    (loss * scale).backward()
    return host(loss), host(w.grad)


@pytest.mark.parametrize("index", range(len(DISTORTION_CASES)))
def test_distortion_loss_value_and_gradient(index):
    n_rays, n_samples = DISTORTION_CASES[index]
    t_np, w_np, scale, (v64, g64), (v32, g32) = distortion_reference(index)
    value, grad = ours_distortion(t_np, w_np, scale)
    what = f"distortion R={n_rays} S={n_samples}"
    within(what + " value", value, v64, v32, n_samples ** 2)
    within(what + " d_weights", grad, g64, g32, n_samples)
    assert np.all(grad[0] == 0)                                    # the ray of zero weights


def test_lossfun_outer_and_lossfun_distortion_per_element():
    from pixie_amd import ray_sampling as rs
    n_rays, n_env, n_fine = 130, 96, 48
    (c_env, w_env), (c, w) = ref.make_level(n_rays, n_env, seed=600), ref.make_level(n_rays, n_fine, seed=601)
    up, up_ray = np.random.default_rng(9).standard_normal((n_rays, n_fine)).astype(F32), np.random.default_rng(10).standard_normal(n_rays).astype(F32)

    def evaluate(dtype):
        t = lambda a: torch.tensor(a, dtype=dtype)
        we, wf = t(w_env[..., 0]).requires_grad_(True), t(w[..., 0]).requires_grad_(True)
        terms, rays = ref.lossfun_outer(t(c), t(w[..., 0]), t(c_env), we), ref.lossfun_distortion(t(c), wf)
        ((terms * t(up)).sum() + (rays * t(up_ray)).sum()).backward()
        return [x.detach().double().numpy() for x in (terms, we.grad, rays, wf.grad)]

    r64, r32 = evaluate(torch.float64), evaluate(torch.float32)
    we, wf = dev(w_env[..., 0]).requires_grad_(True), dev(w[..., 0]).requires_grad_(True)
    terms, rays = rs.lossfun_outer(dev(c), dev(w[..., 0]), dev(c_env), we), rs.lossfun_distortion(dev(c), wf)
    ((terms * dev(up)).sum() + (rays * dev(up_ray)).sum()).backward()
    got = [host(x) for x in (terms, we.grad, rays, wf.grad)]
    for name, g, a, b, terms_ in zip(("lossfun_outer", "lossfun_outer d_w_env", "lossfun_distortion", "lossfun_distortion d_w"), got, r64, r32,
                                     (n_env, n_env, n_fine ** 2, n_fine)):
        within(name + f" R={n_rays}", g, a, b, terms_)


# ---- 8. reproducibility ----------------------------------------------------------------------------------------------------------------
def sample_arrays(s):
    return [host(x) for x in (s.spacing_bins, s.frustums.starts, s.frustums.ends, s.deltas, s.frustums.get_positions())]


@pytest.mark.parametrize("index", [3, 5, 19])                      # 130 rays: single + include_original, single, per-sample
def test_pdf_sampler_is_reproducible(monkeypatch, index):
    case = ref.PDF_CASES[index]
    assert case[0] == 130
    first = sample_arrays(run_pdf(monkeypatch, case, index, "piecewise")[0])
    again = sample_arrays(run_pdf(monkeypatch, case, index, "piecewise")[0])
    order = np.random.default_rng(index).permutation(130)
    permuted = sample_arrays(run_pdf(monkeypatch, case, index, "piecewise", order=order)[0])
    alone = sample_arrays(run_pdf(monkeypatch, case, index, "piecewise", order=np.array([77]))[0])
    for a, b, c, d in zip(first, again, permuted, alone):
        assert bits_equal(a, b) and bits_equal(a[order], c) and bits_equal(a[77:78], d)


def test_spaced_sampler_is_reproducible(monkeypatch):
    from pixie_amd import ray_sampling as rs
    bundle = device_bundle(130, seed=1, near=(0.05, 2.0))
    rand = torch.tensor(np.random.default_rng(2).uniform(0, 1, (130, 97)).astype(F32))
    sampler = rs.UniformLinDispPiecewiseSampler(num_samples=96)

    def run(order):
        fixed_rand(monkeypatch, rand[order])
        idx = torch.as_tensor(order, device=DEV)
        return sample_arrays(sampler(types.SimpleNamespace(**{k: v[idx].contiguous() for k, v in vars(bundle).items()})))

    everyone, order = np.arange(130), np.random.default_rng(3).permutation(130)
    for a, b, c, d in zip(run(everyone), run(everyone), run(order), run(np.array([77]))):
        assert bits_equal(a, b) and bits_equal(a[order], c) and bits_equal(a[77:78], d)


def test_losses_are_reproducible():
    levels, c, w, scale, _, _ = interlevel_reference(2)            # 130 rays, two proposal levels
    order = np.random.default_rng(4).permutation(130)
    (v, g), (v2, g2) = ours_interlevel(levels, c, w, scale), ours_interlevel(levels, c, w, scale)
    _, gp = ours_interlevel(levels, c, w, scale, order)
    _, g1 = ours_interlevel(levels, c, w, scale / 130, np.array([77]))          # alone, R = 1: the same upstream / (R S), exactly 1
    assert bits_equal(v, v2)
    for a, b, p, one in zip(g, g2, gp, g1):
        assert bits_equal(a, b) and bits_equal(a[order], p) and bits_equal(a[77:78], one)
    t_np, w_np, scale, _, _ = distortion_reference(5)              # 130 rays, S = 65
    (v, g), (v2, g2) = ours_distortion(t_np, w_np, scale), ours_distortion(t_np, w_np, scale)
    _, gp = ours_distortion(t_np, w_np, scale, order)
    _, g1 = ours_distortion(t_np, w_np, scale / 130, np.array([77]))
    assert bits_equal(v, v2) and bits_equal(g, g2) and bits_equal(g[order], gp) and bits_equal(g[77:78], g1)
    from pixie_amd import ray_sampling as rs
    rays = host(rs.lossfun_distortion(dev(t_np), dev(w_np[..., 0])))
    assert bits_equal(rays[order], host(rs.lossfun_distortion(dev(t_np[order]), dev(w_np[order, :, 0]))))
    assert bits_equal(rays[77:78], host(rs.lossfun_distortion(dev(t_np[77:78]), dev(w_np[77:78, :, 0]))))


# ---- 9. drop-in ------------------------------------------------------------------------------------------------------------------------
class Blob(torch.nn.Module):
    """an analytic density_fn with parameters: a Gaussian blob of learnable height and centre"""

    def __init__(self, height, centre):
        super().__init__()
        self.height = torch.nn.Parameter(torch.tensor(float(height)))
        self.centre = torch.nn.Parameter(torch.tensor(centre, dtype=torch.float32))

    def forward(self, positions):
        return (torch.nn.functional.softplus(self.height) * torch.exp(-((positions - self.centre) ** 2).sum(-1, keepdim=True) * 0.5) * 4.0).contiguous()


@pytest.mark.parametrize("training", [True, False])
def test_proposal_network_sampler_is_a_drop_in(monkeypatch, training):
    from pixie_amd import ray_render
    from pixie_amd import ray_sampling as rs
    n_rays, levels, n_fine = 130, (256, 96), 48
    bundle = device_bundle(n_rays, seed=21)
    fns = [Blob(1.0, (0.2, -0.1, 0.3)).to(DEV), Blob(0.5, (-0.3, 0.4, 0.0)).to(DEV)]
    sampler = rs.ProposalNetworkSampler(num_proposal_samples_per_ray=levels, num_nerf_samples_per_ray=n_fine, single_jitter=True)
    sampler.train(training)
    drawn, real_rand = [], torch.rand

    def recording_rand(*args, **kwargs):
        drawn.append(real_rand(*args, **kwargs))
        return drawn[-1]

    torch.manual_seed(5)
    with torch.no_grad():
        want_samples, _, want_list = ref.proposal_sample(bundle, fns, levels, n_fine, True, training, DEV)
    want_state = torch.cuda.get_rng_state(DEV)
    torch.manual_seed(5)
    monkeypatch.setattr(torch, "rand", recording_rand)
    samples, weights_list, samples_list = sampler(bundle, fns)
    monkeypatch.setattr(torch, "rand", real_rand)
    assert torch.equal(torch.cuda.get_rng_state(DEV), want_state)
    assert len(drawn) == (3 if training else 0) and len(weights_list) == len(samples_list) == 2
    assert bits_equal(host(samples_list[0].spacing_bins), host(ref.sdist(want_list[0]))), "level-0 bins"
    for k, (previous, weights, produced) in enumerate(zip(samples_list, weights_list, samples_list[1:] + [samples]), start=1):
        n_existing, n_new = weights.shape[1], produced.spacing_bins.shape[1] - 1
        rand = drawn[k].cpu() if training else None
        u = ref.pdf_u(n_new, (n_rays,), rand, torch.float32, "cpu").numpy()
        bins = host(produced.spacing_bins)
        assert np.all(np.diff(bins, axis=1) >= 0)
        worst = ref.pdf_admissible(bins, u, host(previous.spacing_bins), host(weights), 0.01, n_existing)
        note(f"proposal sampler training={training} level {k} ({n_existing} -> {n_new}): share of the allowance used {worst:.3f}")
        assert worst <= 1.0
    assert samples.frustums.starts.shape == (n_rays, n_fine, 1)
    fine_weights = samples.get_weights(fns[1](samples.frustums.get_positions()))
    depth = ray_render.DepthRenderer("expected")(fine_weights, samples)
    assert depth.shape == (n_rays, 1) and torch.isfinite(depth).all()
    loss = rs.interlevel_loss(weights_list + [fine_weights], samples_list + [samples]) + 0.002 * rs.distortion_loss(
        weights_list + [fine_weights], samples_list + [samples])
    want_loss = ref.interlevel_loss(weights_list + [fine_weights], samples_list + [samples]) + 0.002 * ref.distortion_loss(
        weights_list + [fine_weights], samples_list + [samples])
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-5 * max(1.0, abs(float(want_loss.detach())))
    loss.backward()
    for fn in fns:
        assert fn.height.grad is not None and torch.isfinite(fn.height.grad) and fn.centre.grad is not None
    assert float(fns[0].height.grad.abs()) > 0
    # the schedule's other branch: no update this step, the proposal networks run under no_grad
    for fn in fns:
        fn.zero_grad(set_to_none=True)
    sampler.update_sched = lambda step: 5
    sampler.step_cb(20)
    assert sampler._steps_since_update == 1
    _, weights_list, _ = sampler(bundle, fns)
    assert not any(w.requires_grad for w in weights_list) and all(fn.height.grad is None for fn in fns)
    assert sampler._steps_since_update == 1                        # not reset: nothing was updated


# ---- 10. the C API ---------------------------------------------------------------------------------------------------------------------
def test_c_api_refuses_descriptors_outside_the_limits_and_skips_null_outputs():
    from pixie_amd import _lib
    lib = _lib.load()
    ptr = lambda t: t.data_ptr() if t is not None else None
    stream = _lib.current_stream_ptr()
    n_rays, n_samples = 3, 8
    bundle = device_bundle(n_rays)
    table = torch.linspace(0.0, 1.0, n_samples + 1).to(DEV)
    new = lambda *shape: torch.full(shape, -7.0, dtype=torch.float32, device=DEV)
    ins = _lib.RaySampleInputs(ptr(bundle.nears), ptr(bundle.fars), ptr(bundle.origins), ptr(bundle.directions), ptr(table), None, None, None, None, None)
    full = [new(n_rays, n_samples + 1), new(n_rays, n_samples), new(n_rays, n_samples), new(n_rays, n_samples), new(n_rays, n_samples, 3),
            new(n_rays), new(n_rays)]
    desc = lambda **kw: _lib.RaySampleDesc(**{**dict(n_rays=n_rays, n_samples=n_samples, n_existing=0, spacing=4, jitter_stride=0, include_original=0,
                                                     histogram_padding=0.01, eps=1e-5, anneal=1.0, u_scale=0.0, u_offset=0.0), **kw})
    spaced = lambda d, outs: lib.pixie_ray_sample_spaced(C.byref(d), C.byref(ins), C.byref(_lib.RaySampleOutputs(*[ptr(x) for x in outs])), stream)
    assert spaced(desc(), full) == 0
    only_starts = [None, new(n_rays, n_samples), None, None, None, None, None]
    assert spaced(desc(), only_starts) == 0
    torch.cuda.synchronize()
    assert torch.equal(only_starts[1], full[1]) and not (full[0] == -7.0).any() and not (full[4] == -7.0).any()
    untouched = [new(n_rays, n_samples + 1)] + [None] * 6
    for bad in (desc(n_samples=1025), desc(n_samples=0), desc(n_rays=0), desc(n_rays=(1 << 24) + 1), desc(spacing=5), desc(spacing=-1),
                desc(jitter_stride=3)):
        assert spaced(bad, untouched) != 0 and lib.pixie_last_error()
    assert spaced(desc(), [None] * 7) != 0                          # nothing wanted
    edges, weights = ref.make_level(n_rays, 12, seed=1)
    e, w = dev(edges), dev(weights)
    pdf_in = _lib.RaySampleInputs(None, None, None, None, ptr(table), None, ptr(e), ptr(w), ptr(full[5]), ptr(full[6]))
    pdf = lambda d: lib.pixie_ray_sample_pdf(C.byref(d), C.byref(pdf_in), C.byref(_lib.RaySampleOutputs(ptr(untouched[0]), *[None] * 6)), stream)
    for bad in (desc(n_existing=0), desc(n_existing=1025), desc(n_existing=1020, include_original=1), desc(n_samples=1025, n_existing=12)):
        assert pdf(bad) != 0
    level = lambda **kw: _lib.RayInterlevelDesc(**{**dict(n_rays=n_rays, n_fine=12, n_levels=1, n_proposal=(C.c_int32 * 8)(12), per_sample=0), **kw})
    arr = lambda x: (C.c_void_p * 8)(x.data_ptr())
    inter_in = _lib.RayInterlevelInputs(ptr(e), ptr(w), arr(e), arr(w))
    out, scratch, nbytes = new(), new(64), C.c_int64()
    for bad in (level(n_levels=9), level(n_levels=0), level(n_fine=1025), level(n_proposal=(C.c_int32 * 8)(0)), level(n_rays=0)):
        assert lib.pixie_ray_interlevel_forward(C.byref(bad), C.byref(inter_in), ptr(out), None, ptr(scratch), stream) != 0
        assert lib.pixie_ray_interlevel_bytes(C.byref(bad), C.byref(nbytes)) != 0
    assert lib.pixie_ray_interlevel_bytes(C.byref(level()), C.byref(nbytes)) == 0 and nbytes.value == 4 * n_rays
    for bad in (_lib.RayDistortionDesc(n_rays, 0, 0), _lib.RayDistortionDesc(n_rays, 1025, 0), _lib.RayDistortionDesc(0, 12, 0)):
        assert lib.pixie_ray_distortion_forward(C.byref(bad), ptr(e), ptr(w), ptr(out), ptr(scratch), stream) != 0
        assert lib.pixie_ray_distortion_backward(C.byref(bad), ptr(e), ptr(w), ptr(out), ptr(scratch), stream) != 0
    torch.cuda.synchronize()
    assert (untouched[0] == -7.0).all() and float(out) == -7.0 and (scratch == -7.0).all()       # no refused call launched anything
