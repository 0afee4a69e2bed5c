"""CPU checks of pixie_amd/csrc/ray_sample_math.h (compiled for the host by tests/host_harness/ray_sample_math_host.cpp, g++
-ffp-contract=off) against float32 NumPy and the float64 restatement of the reference's lines (tests/_ray_sampling_ref.py), of that
restatement against the reference's own text (tests/golden/ray_sampling.npz), of the device test's admissibility rule on the float32
restatement itself, and of the wrapper's refusals that need no device."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest
import torch

from tests import _ray_render_ref as rref
from tests import _ray_sampling_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "ray_sample_math_host.cpp")
GOLDEN = os.path.join(HERE, "golden", "ray_sampling.npz")
FP = C.POINTER(C.c_float)
F32 = np.float32
KIND = {"uniform": 0, "lindisp": 1, "sqrt": 2, "log": 3, "piecewise": 4}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("rs_host") / "libray_sample_math_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    f = C.c_float
    for name, args in (("spacing_fn", [C.c_int, f]), ("to_euclidean", [C.c_int, f, f, f]), ("delta", [f, f]),
                       ("position", [f, f, f, f]), ("cdf_interp", [f] * 5), ("histogram_weight", [f, f, f])):
        fn = getattr(h, "hh_rs_" + name)
        fn.argtypes, fn.restype = args, f
    h.hh_rs_count_le.argtypes = h.hh_rs_count_lt.argtypes = [FP, C.c_int, f]
    h.hh_rs_stratified_row.argtypes = [FP, C.c_int, FP, C.c_int, FP]
    h.hh_rs_pdf_row.argtypes = [FP, FP, C.c_int, FP, C.c_int, f, f, f, C.c_int, FP, FP]
    h.hh_rs_outer_row.argtypes = [FP, FP, C.c_int, FP, FP, C.c_int, FP, FP, FP]
    h.hh_rs_distortion_row.argtypes = [FP, FP, C.c_int, f, FP]
    h.hh_rs_distortion_row.restype = f
    return h


def ptr(a):
    return a.ctypes.data_as(FP)


def ulps(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


# ---- 1. the restatement is the reference's text ----------------------------------------------------------------------------------------
def test_restatement_equals_the_references_own_text():
    z = np.load(GOLDEN)
    t64 = lambda k: torch.tensor(z[k], dtype=torch.float64)
    edges, weights = t64("edges"), t64("weights")
    s_near, s_far = (ref.SPACING["piecewise"][0](x) for x in (t64("nears"), t64("fars")))
    fn = lambda x: ref.SPACING["piecewise"][1](x * s_far + (1 - x) * s_near)
    existing = types.SimpleNamespace(spacing_starts=edges[..., :-1, None], spacing_ends=edges[..., 1:, None], spacing_to_euclidean_fn=fn)
    bundle = types.SimpleNamespace(origins=torch.zeros(8, 3, dtype=torch.float64), directions=torch.ones(8, 3, dtype=torch.float64))
    levels = {}
    for tag, include, padding in (("train_single", False, 0.01), ("train_each_merged", True, 0.01), ("eval", False, 1e-5), ("eval_merged", True, 0.0)):
        rand = t64(tag + "_rand") if z[tag + "_rand"].size else None
        out = ref.pdf_sample(bundle, existing, weights, 9, rand, include, padding)
        levels[tag] = out
        assert np.max(np.abs(ref.sdist(out).numpy() - z[tag + "_bins"])) <= 1e-14, tag
        assert np.max(np.abs(out.frustums.starts.numpy() - z[tag + "_starts"])) <= 1e-14, tag
        assert np.max(np.abs(out.frustums.ends.numpy() - z[tag + "_ends"])) <= 1e-14, tag
    for tag in ("train_single", "train_each_merged"):
        fine, w_fine = levels[tag], t64(tag + "_fine_weights")
        c = ref.sdist(fine)
        got = {"outer": ref.outer(c[..., :-1], c[..., 1:], edges[..., :-1], edges[..., 1:], weights[..., 0]),
               "lossfun_outer": ref.lossfun_outer(c, w_fine[..., 0], edges, weights[..., 0]),
               "interlevel": ref.interlevel_loss([weights, w_fine], [existing, fine]),
               "lossfun_distortion": ref.lossfun_distortion(c, w_fine[..., 0]),
               "distortion": ref.distortion_loss([weights, w_fine], [existing, fine])}
        for k, v in got.items():
            assert np.max(np.abs(v.numpy() - z[f"{tag}_{k}"])) <= 1e-14, (tag, k)


# ---- 2. the header's rules against float32 NumPy ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_samples", [1, 2, 48, 65, 256])
def test_stratified_bins_are_float32_numpys(host, n_samples):
    rng = np.random.default_rng(n_samples)
    table = torch.linspace(0.0, 1.0, n_samples + 1).numpy()
    for stride in (1, n_samples + 1):
        t = rng.uniform(0, 1, stride).astype(F32)
        got = np.zeros(n_samples + 1, F32)
        host.hh_rs_stratified_row(ptr(table), n_samples, ptr(t), stride, ptr(got))
        want = ref.spaced_bins(n_samples, torch.tensor(t)[None, :], torch.float32, "cpu").numpy()[0]
        centers = (table[1:] + table[:-1]) / F32(2)
        upper, lower = np.r_[centers, table[-1:]], np.r_[table[:1], centers]
        assert bits_equal(got, lower + (upper - lower) * t) and bits_equal(got, want)


def test_spacing_maps_deltas_and_positions(host):
    rng = np.random.default_rng(5)
    x = np.r_[0.0, 1.0, rng.uniform(0, 1, 300)].astype(F32)
    near = np.r_[0.05, 0.999, 1.0, rng.uniform(0.05, 3.0, 299)].astype(F32)        # both sides of 1 for the piecewise kind
    far = (near + np.r_[0.5, 0.002, 4.0, rng.uniform(0.1, 6.0, 299)]).astype(F32)
    one, two, half = F32(1), F32(2), F32(0.5)
    np_fn = {"uniform": (lambda v: v, lambda v: v), "lindisp": (lambda v: one / v, lambda v: one / v),
             "piecewise": (lambda v: np.where(v < one, v / two, one - one / (two * v)), lambda v: np.where(v < half, two * v, one / (two - two * v))),
             "sqrt": (np.sqrt, lambda v: v * v), "log": (np.log, np.exp)}
    for kind, (fn, inv) in np_fn.items():
        k = KIND[kind]
        with np.errstate(divide="ignore", invalid="ignore"):
            s_near, s_far = fn(near).astype(F32), fn(far).astype(F32)
            got_near = np.array([host.hh_rs_spacing_fn(k, v) for v in near], F32)
            got_far = np.array([host.hh_rs_spacing_fn(k, v) for v in far], F32)
            # from the header's own s_near / s_far, so that the inverse is compared on equal operands
            mixed = (x * got_far + (one - x) * got_near).astype(F32)
            want = inv(mixed).astype(F32)
        got = np.array([host.hh_rs_to_euclidean(k, a, b, c) for a, b, c in zip(x, got_near, got_far)], F32)
        if kind in ("sqrt", "log"):
            assert ulps(got_near, s_near).max() <= 2 and ulps(got_far, s_far).max() <= 2 and ulps(got, want).max() <= 2, kind
        else:
            assert bits_equal(got_near, s_near) and bits_equal(got_far, s_far) and bits_equal(got, want), kind
    start, end = near, far
    assert bits_equal([host.hh_rs_delta(a, b) for a, b in zip(start, end)], end - start)
    o, d = rng.uniform(-1, 1, 302).astype(F32), rng.uniform(-1, 1, 302).astype(F32)
    assert bits_equal([host.hh_rs_position(*v) for v in zip(o, d, start, end)], o + d * (start + end) / two)
    want = (torch.tensor(o) + torch.tensor(d) * (torch.tensor(start) + torch.tensor(end)) / 2).numpy()
    assert bits_equal([host.hh_rs_position(*v) for v in zip(o, d, start, end)], want)


def test_cdf_interpolation_given_its_operands(host):
    rng = np.random.default_rng(6)
    c0 = rng.uniform(0, 1, 500).astype(F32)
    c1 = (c0 + rng.uniform(0, 0.2, 500) * (rng.uniform(0, 1, 500) > 0.2)).astype(F32)       # a fifth are flat: 0 / 0 and x / 0
    u = (c0 + (c1 - c0) * rng.uniform(-0.2, 1.2, 500)).astype(F32)
    b0 = rng.uniform(0, 1, 500).astype(F32)
    b1 = (b0 + rng.uniform(0, 0.3, 500)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (u - c0) / (c1 - c0)
    t = np.clip(np.nan_to_num(q, nan=0.0), 0, 1).astype(F32)
    want = b0 + t * (b1 - b0)
    got = [host.hh_rs_cdf_interp(*v) for v in zip(u, c0, c1, b0, b1)]
    assert bits_equal(got, want)
    tt = torch.clip(torch.nan_to_num((torch.tensor(u) - torch.tensor(c0)) / (torch.tensor(c1) - torch.tensor(c0)), 0), 0, 1)
    assert bits_equal(got, (torch.tensor(b0) + tt * (torch.tensor(b1) - torch.tensor(b0))).numpy())
    assert host.hh_rs_cdf_interp(0.5, 0.5, 0.5, 0.25, 0.75) == 0.25 and host.hh_rs_cdf_interp(0.75, 0.5, 0.5, 0.25, 0.75) == 0.75


def test_searchsorted_counts_and_annealing(host):
    rng = np.random.default_rng(7)
    a = np.sort(rng.integers(0, 20, 40)).astype(F32)               # many ties
    for v in np.r_[-1.0, 25.0, rng.integers(0, 20, 30), rng.uniform(0, 20, 30)].astype(F32):
        assert host.hh_rs_count_le(ptr(a), 40, v) == np.searchsorted(a, v, side="right")
        assert host.hh_rs_count_lt(ptr(a), 40, v) == np.searchsorted(a, v, side="left")
    w = rng.uniform(0, 1, 200).astype(F32)
    want = (w.astype(np.float64) ** 0.5).astype(F32)
    assert ulps([host.hh_rs_histogram_weight(v, 0.5, 0.0) for v in w], want).max() <= 2
    assert bits_equal([host.hh_rs_histogram_weight(v, 1.0, 0.01) for v in w], w + F32(0.01))
    assert [host.hh_rs_limit(i) for i in range(2)] == [1024, 8]
    assert [host.hh_rs_samples_per_lane(s) for s in (1, 64, 65, 1024)] == [1, 1, 2, 16]


# ---- 4. the device test's rule, applied to the float32 restatement and to the header's own walk ---------------------------------------
@pytest.mark.parametrize("index", range(len(ref.PDF_CASES)))
def test_admissibility_rule_holds_for_the_float32_restatement(host, index):
    case = ref.PDF_CASES[index]
    n_rays, n_existing, n_new, padding, mode, include = case
    edges, weights, rand, u = ref.pdf_case_inputs(case, index)
    bins = ref.pdf_bins(torch.tensor(edges), torch.tensor(weights), n_new, rand, include, padding).numpy()
    walked = np.zeros_like(bins)
    cdf = np.zeros(n_existing + 1, F32)
    for r in range(n_rays):
        host.hh_rs_pdf_row(ptr(edges[r]), ptr(np.ascontiguousarray(weights[r, :, 0])), n_existing, ptr(np.ascontiguousarray(u[r])), n_new + 1,
                           padding, 1e-5, 1.0, int(include), ptr(cdf), ptr(walked[r]))
    for name, b, share in (("restatement", bins, 0.5), ("header", walked, 1.0)):
        assert np.all(np.diff(b, axis=1) >= 0), name
        fresh = ref.remove_existing(b, edges) if include else b
        assert fresh.shape == (n_rays, n_new + 1)
        worst = ref.pdf_admissible(fresh, u, edges, weights, padding, n_existing)
        assert worst <= share, (name, case, worst)


# ---- the losses' rules, one ray at a time, against float64 autograd --------------------------------------------------------------------
@pytest.mark.parametrize("n_fine,n_env,ties", [(9, 12, False), (48, 96, False), (1, 1, False), (65, 64, False), (150, 49, True)])
def test_outer_walk_against_float64_autograd(host, n_fine, n_env, ties):
    n_rays = 4
    c_env, w_env = ref.make_level(n_rays, n_env, seed=n_fine)
    c, w = ref.make_level(n_rays, n_fine, seed=n_env + 1)
    if ties:                                                       # every proposal edge occurs among the fine edges
        c = np.sort(np.concatenate([c_env, c[:, 1: n_fine - n_env + 1]], axis=1), axis=1)
        assert c.shape[1] == n_fine + 1
    up = np.random.default_rng(8).standard_normal((n_rays, n_fine)).astype(F32)

    def evaluate(dtype):
        t = lambda a: torch.tensor(a, dtype=dtype)
        we = t(w_env[..., 0]).requires_grad_(True)
        terms = ref.lossfun_outer(t(c), t(w[..., 0]), t(c_env), we)
        (terms * t(up)).sum().backward()
        return terms.detach().double().numpy(), we.grad.double().numpy()

    (t64, g64), (t32, g32) = evaluate(torch.float64), evaluate(torch.float32)
    terms, grad = np.zeros((n_rays, n_fine), F32), np.zeros((n_rays, n_env), F32)
    for r in range(n_rays):
        host.hh_rs_outer_row(ptr(c[r]), ptr(np.ascontiguousarray(w[r, :, 0])), n_fine, ptr(c_env[r]), ptr(np.ascontiguousarray(w_env[r, :, 0])),
                             n_env, ptr(up[r]), ptr(terms[r]), ptr(grad[r]))
    assert np.max(np.abs(terms - t64)) <= rref.bar(t64, t32, n_env)
    assert np.max(np.abs(grad - g64)) <= rref.bar(g64, g32, n_env)


@pytest.mark.parametrize("n_samples", [1, 2, 48, 65, 256])
def test_distortion_walk_against_float64_autograd(host, n_samples):
    n_rays = 3
    t_np, w_np = ref.make_level(n_rays, n_samples, seed=n_samples)

    def evaluate(dtype):
        w = torch.tensor(w_np[..., 0], dtype=dtype).requires_grad_(True)
        value = ref.lossfun_distortion(torch.tensor(t_np, dtype=dtype), w)
        value.sum().backward()
        return value.detach().double().numpy(), w.grad.double().numpy()

    (v64, g64), (v32, g32) = evaluate(torch.float64), evaluate(torch.float32)
    value, grad = np.zeros(n_rays, F32), np.zeros((n_rays, n_samples), F32)
    for r in range(n_rays):
        value[r] = host.hh_rs_distortion_row(ptr(t_np[r]), ptr(np.ascontiguousarray(w_np[r, :, 0])), n_samples, 1.0, ptr(grad[r]))
    assert np.max(np.abs(value - v64)) <= rref.bar(v64, v32, n_samples ** 2)
    assert np.max(np.abs(grad - g64)) <= rref.bar(g64, g32, n_samples)


# ---- 3. refusals that need no device ---------------------------------------------------------------------------------------------------
def test_wrapper_refuses_what_it_cannot_run():
    from pixie_amd import ray_sampling as rs
    bundle = ref.make_bundle(4)
    with pytest.raises(ValueError):
        rs.UniformSampler(num_samples=8)(bundle)                   # host tensors: there is no CPU path
    with pytest.raises(ValueError):
        rs.UniformSampler()(None)
    with pytest.raises(ValueError):
        rs.SpacedSampler("cubic")
    with pytest.raises(ValueError):
        rs.PDFSampler(num_samples=8)(bundle, None, torch.zeros(4, 8, 1))
    with pytest.raises(ValueError):
        rs.ProposalNetworkSampler(num_proposal_network_iterations=0)
    with pytest.raises(ValueError):
        rs.lossfun_distortion(torch.zeros(4, 9), torch.zeros(4, 8))
    with pytest.raises(ValueError):
        rs.lossfun_outer(torch.zeros(4, 9), torch.zeros(4, 8), torch.zeros(4, 5), torch.zeros(4, 4))
    with pytest.raises(ValueError):
        rs.interlevel_loss([torch.zeros(4, 8, 1)], [types.SimpleNamespace()])
    with pytest.raises(ValueError):
        rs._limits(1 << 25, 8)
    with pytest.raises(ValueError):
        rs._limits(4, 1025)
    sampler = rs.ProposalNetworkSampler(num_proposal_samples_per_ray=(256, 96), num_nerf_samples_per_ray=48, single_jitter=True)
    assert isinstance(sampler.initial_sampler, rs.UniformLinDispPiecewiseSampler) and sampler.initial_sampler.single_jitter
    assert sampler.pdf_sampler.include_original is False and sampler.pdf_sampler.histogram_padding == 0.01
    sampler.set_anneal(0.5)
    sampler.step_cb(3)
    assert sampler._anneal == 0.5 and sampler._step == 3 and sampler._steps_since_update == 1
    fn = rs.SpacingToEuclidean(rs.SPACING_PIECEWISE, torch.tensor([[0.25]]), torch.tensor([[0.75]]))
    assert torch.equal(fn(torch.tensor([[0.0, 0.5, 1.0]])), torch.tensor([[0.5, 1.0, 2.0]]))
