"""CPU checks of pixie_amd/csrc/ray_render_math.h (compiled for the host by tests/host_harness/ray_render_math_host.cpp, g++
-ffp-contract=off) against the float64 restatement of the reference's lines (tests/_ray_render_ref.py), of that restatement against
the reference's own text (tests/golden/ray_composite.npz), and of the wrapper's refusals that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _ray_render_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "ray_render_math_host.cpp")
GOLDEN = os.path.join(HERE, "golden", "ray_composite.npz")
FP = C.POINTER(C.c_float)
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("rr_host") / "libray_render_math_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    for name, n in (("alpha", 1), ("weight", 2), ("nan_to_num", 1), ("midpoint", 2), ("expected_depth", 2), ("d_depth_d_n", 1),
                    ("d_depth_d_a", 2), ("d_depth_d_weight", 3)):
        fn = getattr(h, "hh_rr_" + name)
        fn.argtypes, fn.restype = [C.c_float] * n, C.c_float
    h.hh_rr_replaced.argtypes = [C.c_float]
    h.hh_rr_median_index.argtypes = [FP, C.c_int]
    h.hh_rr_ray_forward.argtypes = [FP, FP, FP, FP, C.c_int, FP, FP, FP]
    h.hh_rr_ray_backward.argtypes = [FP, FP, FP, C.c_int, FP]
    return h


def ptr(a):
    return a.ctypes.data_as(FP)


def test_nan_to_num_is_torchs_full_rule(host):
    cases = [np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1.5, -2.5, FLT_MAX, -FLT_MAX, 1e-45, -1e-45]
    want = torch.nan_to_num(torch.tensor(cases, dtype=torch.float32)).numpy()
    got = np.array([host.hh_rr_nan_to_num(v) for v in cases], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert [host.hh_rr_replaced(v) for v in cases] == [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert want[2] == FLT_MAX and want[3] == -FLT_MAX and want[0] == 0


def test_weight_and_special_values(host):
    rng = np.random.default_rng(0)
    x = np.exp(rng.uniform(np.log(1e-6), np.log(50.0), 400)).astype(F32)
    prefix = np.exp(rng.uniform(np.log(1e-6), np.log(50.0), 400)).astype(F32)
    for xi, pi in zip(x, prefix):
        want = (1.0 - np.exp(-float(xi))) * np.exp(-float(pi))
        # alpha: expf to an ulp and one subtraction, absolute error <= 2 u; times a transmittance good to a few ulp
        assert abs(host.hh_rr_weight(xi, pi) - want) <= 4 * U * np.exp(-float(pi)) + 4 * U * want, (xi, pi)
        assert abs(host.hh_rr_alpha(xi) - (1.0 - np.exp(-float(xi)))) <= 2 * U
    assert host.hh_rr_weight(0.0, 0.0) == 0.0 and host.hh_rr_weight(0.0, 3.0) == 0.0
    assert host.hh_rr_weight(np.inf, 0.0) == 1.0 and host.hh_rr_weight(1e4, 0.0) == 1.0
    assert host.hh_rr_weight(1.0, np.inf) == 0.0
    assert host.hh_rr_weight(np.nan, 0.0) == 0.0 and host.hh_rr_weight(1.0, np.nan) == 0.0
    assert host.hh_rr_weight(-np.inf, 0.0) == -FLT_MAX            # alpha = 1 - exp(inf) = -inf, replaced by nan_to_num
    assert host.hh_rr_midpoint(1.0, 2.0) == 1.5
    a = F32(0.1) + F32(0.7)
    assert host.hh_rr_midpoint(0.1, 0.7) == float(F32(a) / F32(2))


def test_depth_quotient_and_its_derivatives(host):
    rng = np.random.default_rng(1)
    for a, n in zip(np.r_[0.0, 1e-12, rng.uniform(1e-3, 1, 50)].astype(F32), np.r_[0.0, 1e-12, rng.uniform(0, 4, 50)].astype(F32)):
        d = F32(a) + F32(1e-10)
        assert host.hh_rr_expected_depth(n, a) == float(F32(n) / d)
        assert host.hh_rr_d_depth_d_n(a) == float(F32(1) / d)
        assert host.hh_rr_d_depth_d_a(n, a) == float(-F32(n) / F32(d * d))
        if a > 1e-3:
            A, N = float(a), float(n)
            h = 1e-6
            assert abs(host.hh_rr_d_depth_d_n(a) - 1 / (A + 1e-10)) <= 4 * U / A
            assert abs(host.hh_rr_d_depth_d_a(n, a) - ((N / (A + h + 1e-10) - N / (A - h + 1e-10)) / (2 * h))) <= 1e-4 * (1 + N / A ** 2)
    assert host.hh_rr_expected_depth(0.0, 0.0) == 0.0             # the all-zero ray: 0 / 1e-10, not NaN
    assert host.hh_rr_d_depth_d_weight(2.0, 0.5, -0.25) == 0.75


def test_median_rule(host):
    def med(w):
        w = np.asarray(w, F32)
        return host.hh_rr_median_index(ptr(w), len(w))
    assert med([0.5]) == 0 and med([0.1]) == 0
    assert med([0.25, 0.25, 0.5]) == 1                            # the running sum reaches 0.5 exactly: side="left"
    assert med([0.25, 0.2, 0.5]) == 2
    assert med([0.1, 0.1, 0.1]) == 2                              # never reached: clamped to S - 1
    assert med([0.0, 0.0, 0.0, 0.0]) == 3
    assert med([0.6, 0.3]) == 0
    rng = np.random.default_rng(2)
    for trial in range(50):
        n = int(rng.integers(1, 200))
        w = (rng.uniform(0, 1, n) ** 4 * rng.uniform(0, 3) / n).astype(F32)
        cum = torch.cumsum(torch.tensor(w), 0)                    # sequential float32 on the CPU for these lengths
        seq = np.float32(0)
        first = n
        for i in range(n):
            seq = np.float32(seq + w[i])
            if first == n and seq >= 0.5:
                first = i
        assert med(w) == min(first, n - 1), trial
        ok = ref.median_admissible(np.array([(F32(i) + F32(i + 1)) / F32(2) for i in [med(w)]], F32), w.astype(np.float64)[None, :, None],
                                   np.arange(n, dtype=F32)[None, :, None], np.arange(1, n + 1, dtype=F32)[None, :, None], n)
        assert ok.all(), trial


def test_ray_walk_against_the_float64_restatement(host):
    """one ray walked with the header's rules: weights, accumulation, expected depth and d_density under _ray_render_ref.bar"""
    for n, seed in ((1, 0), (2, 1), (48, 2), (65, 3), (256, 4), (1024, 5)):
        inp = ref.make_inputs(6, n, 0, seed=seed, rgb=False)
        up = ref.make_upstream(6, n, 0, seed=seed + 100, rgb=False)
        up["accumulation"] = up["expected_depth"] = None          # g = the weights' upstream gradient alone
        (o64, g64), (o32, g32) = ref.evaluate(inp, up, torch.float64), ref.evaluate(inp, up, torch.float32)
        ex64 = ref.expected_depth(torch.tensor(o64["weights"]), torch.tensor(inp["starts"], dtype=torch.float64),
                                  torch.tensor(inp["ends"], dtype=torch.float64), clip=False).numpy()
        ex32 = ref.expected_depth(torch.tensor(o32["weights"], dtype=torch.float32), torch.tensor(inp["starts"]), torch.tensor(inp["ends"]),
                                  clip=False).double().numpy()
        w, d = np.zeros((6, n), F32), np.zeros((6, n), F32)
        acc, dep = np.zeros((6, 1), F32), np.zeros((6, 1), F32)
        for r in range(6):
            flat = {k: np.ascontiguousarray(inp[k][r, :, 0]) for k in ("deltas", "densities", "starts", "ends")}
            a, e = C.c_float(), C.c_float()
            host.hh_rr_ray_forward(ptr(flat["deltas"]), ptr(flat["densities"]), ptr(flat["starts"]), ptr(flat["ends"]), n, ptr(w[r]), C.byref(a),
                                   C.byref(e))
            acc[r], dep[r] = a.value, e.value
            g = np.ascontiguousarray(up["weights"][r, :, 0])
            host.hh_rr_ray_backward(ptr(flat["deltas"]), ptr(flat["densities"]), ptr(g), n, ptr(d[r]))
        for name, got, r64, r32, terms in (("weights", w[..., None], o64["weights"], o32["weights"], n),
                                           ("accumulation", acc, o64["accumulation"], o32["accumulation"], n),
                                           ("expected_depth", dep, ex64, ex32, n),
                                           ("d_density", d[..., None], g64["densities"], g32["densities"], n)):
            err = float(np.max(np.abs(got.astype(np.float64) - r64)))
            assert err <= ref.bar(r64, r32, terms), (n, name, err, ref.bar(r64, r32, terms))


def test_nan_density_masks_the_rest_of_the_ray(host):
    n, k = 12, 5
    inp = ref.make_inputs(1, n, 0, seed=9, rgb=False)
    delta, sigma = np.ascontiguousarray(inp["deltas"][0, :, 0]), np.ascontiguousarray(inp["densities"][0, :, 0])
    clean = sigma.copy()
    sigma[k] = np.nan
    g = np.random.default_rng(3).standard_normal(n).astype(F32)
    w, d = np.zeros(n, F32), np.zeros(n, F32)
    a, e = C.c_float(), C.c_float()
    z = np.zeros(n, F32)
    host.hh_rr_ray_forward(ptr(delta), ptr(sigma), ptr(z), ptr(z), n, ptr(w), C.byref(a), C.byref(e))
    want = ref.get_weights(torch.tensor(sigma)[None, :, None], torch.tensor(delta)[None, :, None])[0, :, 0].numpy()
    assert np.all(w[k:] == 0) and np.all(want[k:] == 0) and np.all(w[:k] > 0)
    host.hh_rr_ray_backward(ptr(delta), ptr(sigma), ptr(g), n, ptr(d))
    assert np.all(np.isfinite(d)) and np.all(d[k:] == 0)
    keep = (np.arange(n) < k).astype(np.float64)[None, :, None]
    cut = {"densities": clean[None, :, None], "deltas": delta[None, :, None], "starts": z[None, :, None], "ends": z[None, :, None]}
    up = {"weights": g[None, :, None]}
    (_, g64), (_, g32) = ref.evaluate(cut, up, torch.float64, keep=keep), ref.evaluate(cut, up, torch.float32, keep=keep)
    err = float(np.max(np.abs(d[:k] - g64["densities"][0, :k, 0])))
    assert err <= ref.bar(g64["densities"], g32["densities"], n), err


def test_restatement_equals_the_references_own_text():
    """tests/golden/ray_composite.npz: the reference's functions, cut out of its source and run in float64 (make_ray_composite_golden.py)"""
    z = np.load(GOLDEN)
    t = {k: torch.tensor(z[k], dtype=torch.float64) for k in ("densities", "deltas", "starts", "ends", "rgb", "features")}
    w = ref.get_weights(t["densities"], t["deltas"])
    got = {"weights": w, "rgb_random": ref.combine_rgb(t["rgb"], w, "random"), "rgb_last_sample": ref.combine_rgb(t["rgb"], w, "last_sample"),
           "rgb_white": ref.combine_rgb(t["rgb"], w, "white"), "accumulation": ref.accumulation(w),
           "median_depth": ref.median_depth(w, t["starts"], t["ends"]), "expected_depth": ref.expected_depth(w, t["starts"], t["ends"]),
           "feature": ref.feature(t["features"], w)}
    for k, v in got.items():
        assert np.max(np.abs(v.numpy() - z["out_" + k])) <= 1e-14, k


def test_wrapper_refuses_what_it_cannot_run():
    from pixie_amd import ray_render
    w = torch.zeros(2, 4, 1)
    with pytest.raises(ValueError):
        ray_render.get_weights(w, w)                                # host tensors: there is no CPU path
    with pytest.raises(ValueError):
        ray_render.AccumulationRenderer.forward(w)
    with pytest.raises(NotImplementedError):
        ray_render.AccumulationRenderer.forward(w, ray_indices=torch.zeros(8, dtype=torch.long), num_rays=2)
    with pytest.raises(NotImplementedError):
        ray_render.RGBRenderer.combine_rgb(torch.zeros(2, 4, 3), w, ray_indices=torch.zeros(8, dtype=torch.long), num_rays=2)
    with pytest.raises(NotImplementedError):
        ray_render.DepthRenderer("mean")
    with pytest.raises(ValueError):
        ray_render._background("magenta")
    assert ray_render._background("white") == (1, (1.0, 1.0, 1.0)) and ray_render._background("random")[0] == 0
    assert ray_render._background(torch.tensor([0.1, 0.2, 0.3]))[0] == 1 and ray_render._background("last_sample")[0] == 2


def test_header_limits_match_the_binding(host):
    from pixie_amd import _lib
    assert [host.hh_rr_limit(i) for i in range(4)] == [_lib.RAY_MAX_SAMPLES, _lib.RAY_MAX_FEATURE_SAMPLES, _lib.RAY_MAX_CHANNELS, 256]
    assert [host.hh_rr_samples_per_lane(s) for s in (1, 64, 65, 1000, 1024)] == [1, 1, 2, 16, 16]
    assert [host.hh_rr_chunks(c) for c in (0, 4, 256, 260, 768, 2048)] == [0, 1, 1, 2, 3, 8]
