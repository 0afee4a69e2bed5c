"""CPU checks of pixie_amd/csrc/raster_math.h (compiled for the host by tests/host_harness/raster_math_host.cpp, g++
-ffp-contract=off) against the float64 run of tests/_raster_ref.py.

Bars.  Radius and tile rectangle: exact off the borderline Gaussians.  Depth, centre and conic: let y be the largest error of the
helper's own float32 run against its float64 run (off the borderline set); the header must lie within 3 y of the float64 run.
The factor 3 leaves room for a different but equally valid float32 rounding sequence; it is not derived from the header's output."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _raster_ref as rr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "raster_math_host.cpp")
FP = C.POINTER(C.c_float)


def fp(a):
    return a.ctypes.data_as(FP) if a is not None else None


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("raster_host") / "libraster_math_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_raster_project.argtypes = [C.c_int, FP, FP, FP, FP, C.c_float, FP, FP, C.c_float, C.c_float, C.c_int, C.c_int, FP, C.POINTER(C.c_int)]
    h.hh_raster_cov3d.argtypes = [C.c_int, FP, FP, C.c_float, FP]
    h.hh_raster_blend.argtypes = [C.c_int, FP, C.c_float, C.c_float, FP, FP]
    h.hh_raster_sh.argtypes = [C.c_int, C.c_int, C.c_int, FP, FP, FP]
    return h


def host_project(h, means, cam, cov6=None, scales=None, rotations=None, mod=1.0):
    n = len(means)
    means = np.ascontiguousarray(means, np.float32)
    arrs = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (cov6, scales, rotations)]
    of, oi = np.zeros((n, 6), np.float32), np.zeros((n, 5), np.int32)
    V, P = np.ascontiguousarray(cam["V"], np.float32).reshape(16), np.ascontiguousarray(cam["P"], np.float32).reshape(16)
    h.hh_raster_project(n, fp(means), fp(arrs[0]), fp(arrs[1]), fp(arrs[2]), mod, fp(V), fp(P), cam["tanfovx"], cam["tanfovy"], cam["W"], cam["H"],
                        fp(of), oi.ctypes.data_as(C.POINTER(C.c_int)))
    return of, oi


def random_case(k):
    rng = np.random.default_rng(1000 + k)
    s = rr._cloud(rng, 1000, (0, 0, 0), (1.5, 1.5, 1.5), 0.005, 0.2)
    eye = rng.normal(size=3)
    eye = eye / np.linalg.norm(eye) * rng.uniform(1.0, 5.0)          # some cameras sit inside the cloud: culls and clamps occur
    W, H = int(rng.integers(40, 900)), int(rng.integers(40, 700))
    s["cam"] = rr.look_at_camera(eye, rng.normal(size=3) * 0.3, float(rng.uniform(30, 120)), W, H, up=(0.1, 1.0, 0.2))
    s["scale_modifier"] = float(rng.uniform(0.5, 1.5))
    return s


def test_projection_against_the_float64_helper(host):
    """10 cameras x 1000 Gaussians: radius and rectangle exact, depth / centre / conic within 3 y (see the module docstring)"""
    worst, total, border, culled, clamped = {}, 0, 0, 0, 0
    for k in range(10):
        s = random_case(k)
        cam = s["cam"]
        c32 = rr.cov3d_from_scale_rot(s["scales"], s["rotations"], s["scale_modifier"], np.float32)
        p64 = rr.project(s["means"], c32, cam, np.float64)
        p32 = rr.project(s["means"], c32, cam, np.float32)
        of, oi = host_project(host, s["means"], cam, cov6=c32)
        keep = ~p64["borderline"]
        total, border, culled = total + len(keep), border + int((~keep).sum()), culled + int((~p64["valid"]).sum())
        assert np.array_equal(oi[keep, 0], p64["radius"][keep]), f"case {k}: radius"
        assert np.array_equal(oi[keep, 1:], p64["rect"][keep]), f"case {k}: rectangle"
        v = keep & p64["valid"] & p32["valid"]
        for name, got, idx in (("depth", of[:, 0], "depth"), ("px", of[:, 1], "px"), ("py", of[:, 2], "py")):
            y = np.max(np.abs(p32[idx][v].astype(np.float64) - p64[idx][v]) / np.maximum(np.abs(p64[idx][v]), 1.0))
            e = np.max(np.abs(got[v].astype(np.float64) - p64[idx][v]) / np.maximum(np.abs(p64[idx][v]), 1.0))
            worst[name] = max(worst.get(name, 0.0), e / max(y, 2.0 ** -24))
            assert e <= 3 * max(y, 2.0 ** -24), (k, name, e, y)
        scale = np.max(np.abs(p64["conic"][v]), axis=1, keepdims=True)
        y = np.max(np.abs(p32["conic"][v].astype(np.float64) - p64["conic"][v]) / scale)
        e = np.max(np.abs(of[v, 3:6].astype(np.float64) - p64["conic"][v]) / scale)
        worst["conic"] = max(worst.get("conic", 0.0), e / y)
        assert e <= 3 * y, (k, "conic", e, y)
        # the scale / rotation route builds the same covariance
        of2, oi2 = host_project(host, s["means"], cam, scales=s["scales"], rotations=s["rotations"], mod=s["scale_modifier"])
        assert np.array_equal(oi2[keep], oi[keep])
    print(f"{total} Gaussians, {culled} culled, {border} borderline; error over the float32 helper's: " +
          ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert border <= 0.005 * total and 0.02 * total < culled < 0.9 * total


def test_isotropic_gaussian_on_the_optical_axis():
    """cov2D = sigma^2 f^2 / z^2 + 0.3 on both diagonal entries, 0 off it"""
    cam = rr.look_at_camera((0, 0, -4.0), (0, 0, 0), 60.0, 320, 320)
    sigma, z = 0.05, 4.0
    f = cam["W"] / (2 * np.tan(np.radians(60.0) / 2))
    cov = np.array([[sigma ** 2, 0, 0, sigma ** 2, 0, sigma ** 2]])
    p = rr.project(np.zeros((1, 3)), cov, cam, np.float64)
    want = sigma ** 2 * f ** 2 / z ** 2 + 0.3
    assert np.allclose(p["cov2d"][0], [want, 0.0, want], rtol=1e-6, atol=1e-9)
    assert np.allclose([p["px"][0], p["py"][0]], [159.5, 159.5], atol=1e-4) and p["radius"][0] == int(np.ceil(3 * np.sqrt(want)))


def test_isotropic_gaussian_through_the_header(host):
    cam = rr.look_at_camera((0, 0, -4.0), (0, 0, 0), 60.0, 320, 320)
    sigma = 0.05
    f = cam["W"] / (2 * np.tan(np.radians(60.0) / 2))
    want = sigma ** 2 * f ** 2 / 16.0 + 0.3
    of, oi = host_project(host, np.zeros((1, 3)), cam, scales=np.full((1, 3), sigma), rotations=np.array([[1.0, 0, 0, 0]]))
    assert np.allclose(of[0, 3:6], [1 / want, 0.0, 1 / want], rtol=1e-5, atol=1e-7) and abs(of[0, 0] - 4.0) < 1e-5
    assert oi[0, 0] == int(np.ceil(3 * np.sqrt(want))) and np.allclose(of[0, 1:3], 159.5, atol=1e-3)


def test_the_clamp_at_1p3_tanfov(host):
    """far off axis, t.x / t.z enters the Jacobian as +-1.3 tanfov: moving the Gaussian further out along x changes its 2D covariance
    no more (same depth), while inside the clamp it does"""
    cam = rr.look_at_camera((0, 0, 0.0), (0, 0, 1.0), 60.0, 200, 200)
    lim = 1.3 * cam["tanfovx"]
    z = 2.0
    xs = np.array([0.5 * lim * z, 0.9 * lim * z, 1.5 * lim * z, 3.0 * lim * z, lim * z, -lim * z, -2.0 * lim * z])
    means = np.stack([xs, np.zeros(7), np.full(7, z)], axis=1)
    cov = np.tile(np.array([[0.02, 0.001, 0.002, 0.03, 0.001, 0.01]]), (7, 1))
    p = rr.project(means, cov, cam, np.float64)
    assert np.allclose(p["cov2d"][2], p["cov2d"][3], rtol=1e-12) and not np.allclose(p["cov2d"][0], p["cov2d"][1], rtol=1e-3)
    assert np.allclose(p["cov2d"][4], p["cov2d"][3], rtol=1e-6)        # ... and it is the covariance of the Gaussian AT the limit
    assert np.allclose(p["cov2d"][5], p["cov2d"][6], rtol=1e-6) and not np.allclose(p["cov2d"][5], p["cov2d"][4], rtol=1e-3)
    of, _ = host_project(host, means, cam, cov6=cov)
    assert np.allclose(of[2, 3:6], of[3, 3:6], rtol=1e-6)


def test_sh_evaluation(host):
    rng = np.random.default_rng(5)
    n = 2000
    shs = rng.normal(size=(n, 16, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    for degree in range(4):
        got = np.zeros((n, 3), np.float32)
        host.hh_raster_sh(n, 16, degree, fp(shs), fp(d), fp(got))
        want = rr.eval_sh64(shs, degree, d)
        assert np.allclose(got, want, rtol=0, atol=4e-6), degree       # 16 terms of size <= ~4 in float32
        if degree:
            assert not np.allclose(got, rr.eval_sh64(shs, degree - 1, d), atol=1e-3)
    c = rng.uniform(-1, 1, size=(n, 16, 3)).astype(np.float32)          # degree 0 gives 0.2820948 c + 0.5
    got = np.zeros((n, 3), np.float32)
    host.hh_raster_sh(n, 16, 0, fp(c), fp(d), fp(got))
    assert np.allclose(got, np.maximum(0.2820948 * c[:, 0].astype(np.float64) + 0.5, 0), rtol=0, atol=2e-7)


def blend_ref(g, pix, bg, dtype):
    """the helper's blend over a hand-made sorted list: a one-pixel scene is not needed, the rules are applied directly"""
    f = dtype
    T, Cc, last = f(1), np.zeros(3, f), 0
    for k, q in enumerate(np.asarray(g).astype(f)):
        dx, dy = q[0] - f(pix[0]), q[1] - f(pix[1])
        power = f(-0.5) * (q[2] * dx * dx + q[4] * dy * dy) - q[3] * dx * dy
        if power > 0:
            continue
        alpha = min(f(0.99), q[5] * np.exp(power))
        if alpha < f(1.0) / f(255.0):
            continue
        test_T = T * (f(1) - alpha)
        if test_T < f(0.0001):
            break
        Cc = Cc + q[6:9] * (alpha * T)
        T, last = test_T, k + 1
    return np.concatenate([Cc + T * np.asarray(bg).astype(f), [T, last]])


def test_blend_over_a_sorted_list(host):
    """early termination, the 0.99 clamp, the 1/255 skip and the power > 0 skip, against the helper's rules in float64"""
    rng = np.random.default_rng(9)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    for case in range(200):
        n = int(rng.integers(1, 40))
        g = np.zeros((n, 9), np.float32)
        g[:, 0:2] = rng.normal(size=(n, 2)) * 3 + 8
        a, c = rng.uniform(0.02, 0.5, n), rng.uniform(0.02, 0.5, n)
        g[:, 2], g[:, 4] = a, c
        g[:, 3] = rng.uniform(-1.2, 1.2, n) * np.sqrt(a * c)            # |b| > sqrt(ac): indefinite, power > 0 occurs
        g[:, 5] = rng.choice([0.01, 0.3, 0.99, 1.0, 5.0], n)            # 5.0: alpha clamps at 0.99
        g[:, 6:9] = rng.uniform(0, 1, (n, 3))
        out = np.zeros(5, np.float32)
        host.hh_raster_blend(n, fp(g), 8.0, 8.0, fp(bg), fp(out))
        r64, r32 = blend_ref(g, (8.0, 8.0), bg, np.float64), blend_ref(g, (8.0, 8.0), bg, np.float32)
        if r64[4] != r32[4]:
            continue                                                    # a borderline list: float32 itself takes another branch
        assert out[4] == r64[4], case
        y = max(np.max(np.abs(r32[:4] - r64[:4])), 2.0 ** -24)
        assert np.max(np.abs(out[:4] - r64[:4])) <= 3 * y, case
    # a stack of opaque Gaussians stops at the second: T = 0.01 after one, 1e-4 is not < 1e-4 in exact arithmetic but the third always is
    g = np.zeros((5, 9), np.float32)
    g[:, 0:2], g[:, 2], g[:, 4], g[:, 5] = 8.0, 0.1, 0.1, 1.0
    g[:, 6] = [1, 0, 0, 0, 0]
    g[:, 7] = [0, 1, 0, 0, 0]
    out = np.zeros(5, np.float32)
    host.hh_raster_blend(5, fp(g), 8.0, 8.0, fp(bg), fp(out))
    assert out[4] in (1.0, 2.0) and np.isclose(out[0], 0.99 + out[3] * 0.1, atol=1e-6) and out[3] <= 0.0100001
