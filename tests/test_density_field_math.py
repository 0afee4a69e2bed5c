"""CPU checks of pixie_amd/csrc/density_field_math.h (compiled for the host by tests/host_harness/density_field_math_host.cpp, g++
-ffp-contract=off): the front end's bits against the NumPy restatement, the 16-wide fmaf chains against float64 within the suite's
bar, trunc_exp's derivative rule, and the host policy (slabs, launch geometry, byte sizes) against a Python restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _density_field_ref as D
from tests import _field_query_ref as R
from tests import _hashmlp_grad_ref as G

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "density_field_math_host.cpp")
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int)
LEVEL = np.dtype([("scale", "f4"), ("shift", "f4"), ("res", "u4"), ("size", "u4"), ("offset", "u4"), ("dense", "u4")])
NS = [1, 64, 65, 2 ** 20, 2 ** 24]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("df_host") / "libdensity_field_math_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_df_forward.argtypes = [C.c_void_p, C.c_int, C.c_int, FP] + [C.c_int] + [FP] * 6 + [FP, C.c_int, FP, FP, C.c_int64, FP, FP, IP]
    h.hh_df_forward.restype = None
    h.hh_df_density.argtypes, h.hh_df_density.restype = [C.c_float, C.c_float], C.c_float
    h.hh_df_dh.argtypes, h.hh_df_dh.restype = [C.c_float, C.c_float, C.c_float, C.c_int], C.c_float
    for name in ("hh_df_forward_blocks", "hh_df_slab_count"):
        getattr(h, name).argtypes = [C.c_int64]
    h.hh_df_param_count.argtypes = [C.c_int, C.c_int]
    h.hh_df_weight_offset.argtypes = [C.c_int, C.c_int, C.c_int]
    h.hh_df_saved_bytes.argtypes, h.hh_df_saved_bytes.restype = [C.c_int64], C.c_int64
    h.hh_df_scratch.argtypes, h.hh_df_scratch.restype = [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_int64)], None
    return h


def fp(a):
    return None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(FP)


def host_forward(host, net, x32, front):
    lv = np.array([tuple(l[k] for k in LEVEL.names) for l in net["levels"]], LEVEL)
    n, nh = len(x32), len(net["weights"]) - 1
    ws = [np.ascontiguousarray(w, np.float32) for w in net["weights"]] + [None] * (2 - nh)
    bs = [None if net["biases"] is None else np.ascontiguousarray(b, np.float32) for b in (net["biases"] or [None] * (nh + 1))] + [None] * (2 - nh)
    table = np.ascontiguousarray(net["table"], np.float32)
    x = np.ascontiguousarray(x32, np.float32)
    A = front.get("world_to_nerf")
    A = None if A is None else np.ascontiguousarray(np.asarray(A, np.float32)[:3])
    aabb = np.ascontiguousarray(np.asarray(front.get("aabb", [[-1] * 3, [1] * 3]), np.float32).reshape(-1))
    h, p, sel = np.empty(n, np.float32), np.empty((n, 3), np.float32), np.empty(n, np.int32)
    host.hh_df_forward(lv.ctypes.data, len(lv), net["F"], fp(table), nh, *[fp(w) for w in ws], *[fp(b) for b in bs], fp(A),
                       int(front.get("contraction", True)), fp(aabb), fp(x), n, h.ctypes.data_as(FP), p.ctypes.data_as(FP), sel.ctypes.data_as(IP))
    return h, p, sel


FRONTS = {
    "contraction": dict(contraction=True),
    "aabb": dict(contraction=False, aabb=[[-2.0, -1.5, -2.5], [2.0, 2.5, 1.5]]),
    "affine": dict(contraction=True, world_to_nerf=[[0.9, 0.1, -0.2, 0.05], [-0.1, 1.1, 0.3, -0.2], [0.2, -0.3, 0.8, 0.1]]),
}
NETS = {
    "ns_5xF2_h1": ("nerfstudio", 5, 16, 128, 12, 2, 1, True),
    "tcnn_5xF2_h1_nobias": ("tcnn", 5, 16, 128, 12, 2, 1, False),
    "ns_7xF2_h2": ("nerfstudio", 7, 16, 2048, 10, 2, 2, True),
    "tcnn_3xF4_h1": ("tcnn", 3, 16, 64, 8, 4, 1, True),
    "linear": ("nerfstudio", 5, 16, 128, 12, 2, 0, True),
}


def points(rng, n):
    x = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    x[:6] = [[0, 0, 0], [1, 0.5, -0.25], [-1, 1, 1], [2, 2, 2], [0.5, -0.999, 0.25], [1e-30, 0, 0]]     # m exactly 1 takes the contraction branch
    return x


@pytest.mark.parametrize("front", sorted(FRONTS))
def test_front_end_bits(host, front):
    rng = np.random.default_rng(5)
    net = D.random_net(rng, *NETS["ns_5xF2_h1"])
    x = points(rng, 500)
    _, p, sel = host_forward(host, net, x, FRONTS[front])
    f = FRONTS[front]
    A = np.eye(4, dtype=np.float32)[:3] if f.get("world_to_nerf") is None else np.asarray(f["world_to_nerf"], np.float32)
    want_p, want_sel = R.world_to_unit(x, A, f["contraction"], f.get("aabb"))
    assert np.array_equal(p.view(np.uint32), want_p.view(np.uint32))
    assert np.array_equal(sel.astype(bool), want_sel)
    assert 0 < want_sel.sum() < len(x) or front != "aabb"


def test_nan_coordinate_has_selector_zero(host):
    net = D.random_net(np.random.default_rng(6), *NETS["ns_5xF2_h1"])
    x = np.array([[np.nan, 0.1, 0.2], [0.1, np.nan, 0.2], [0.1, 0.2, np.nan], [0.1, 0.2, 0.3]], np.float32)
    h, _, sel = host_forward(host, net, x, FRONTS["contraction"])
    assert list(sel) == [0, 0, 0, 1] and np.all(np.isfinite(h)), "a masked point is evaluated at p = 0"
    assert h[0].view(np.uint32) == h[1].view(np.uint32) == h[2].view(np.uint32)


@pytest.mark.parametrize("name", sorted(NETS))
def test_h_within_the_bar(host, name):
    rng = np.random.default_rng(sum(map(ord, name)))
    net = D.random_net(rng, *NETS[name])
    x = points(rng, 600)
    front = FRONTS["contraction"]
    h, _, _ = host_forward(host, net, x, front)
    zero = np.zeros(len(x))
    ref = D.evaluate(net, x, zero, torch.float64, front)["h"]
    yard = D.evaluate(net, x, zero, torch.float32, front)["h"]
    limit = G.bar(ref, yard, [net])
    err = np.abs(h.astype(np.float64) - ref).max()
    print(f"{name}: max|h - f64| {err:.3e}, float32 torch {np.abs(yard - ref).max():.3e}, bar {limit:.3e}")
    assert err <= limit


def test_derivative_rule(host):
    for aid in (1.0, 0.01, 2.5):
        for h in (-20.0, -15.0, 0.0, 15.0, 20.0, 89.0):
            for g in (1.0, -0.37, 3.0e4):
                want = np.float64(np.float32(g)) * np.float64(np.float32(aid)) * np.exp(np.clip(np.float64(h), -15, 15))
                got = host.hh_df_dh(g, h, aid, 1)
                assert abs(got - want) <= 4 * 2.0 ** -24 * abs(want), (aid, h, g, got, want)
                assert host.hh_df_dh(g, h, aid, 0) == 0.0
            d = host.hh_df_density(h, aid)
            if h > 88.8:
                assert d == np.inf
            else:
                assert abs(d - aid * np.exp(np.float64(h))) <= 4 * 2.0 ** -24 * aid * np.exp(np.float64(h))
    e15 = host.hh_df_dh(1.0, 89.0, 1.0, 1)
    assert e15 == host.hh_df_dh(1.0, 15.0, 1.0, 1) == host.hh_df_dh(1.0, 20.0, 1.0, 1) and abs(e15 - np.exp(15.0)) < 1.0
    assert host.hh_df_dh(1.0, -20.0, 1.0, 1) == host.hh_df_dh(1.0, -15.0, 1.0, 1) > 0


def py_slabs(n):
    return max(1, min(-(-n // 256), 1024))


def py_params(in_dim, nh):
    return in_dim + 1 if nh == 0 else 16 * in_dim + 16 + (nh - 1) * (256 + 16) + 16 + 1


def test_policy_against_python(host):
    r256 = lambda b: -(-b // 256) * 256
    for n in NS:
        assert host.hh_df_slab_count(n) == py_slabs(n)
        assert host.hh_df_forward_blocks(n) == max(1, min(-(-n // 256), 2048))
        assert host.hh_df_saved_bytes(n) == 0
        for in_dim, nh, rows, F in ((10, 1, 5 << 17, 2), (14, 2, 7 << 10, 2), (12, 1, 3 << 8, 4), (10, 0, 5 << 12, 2), (64, 2, 1 << 20, 8)):
            assert host.hh_df_param_count(in_dim, nh) == py_params(in_dim, nh)
            out = (C.c_int64 * 5)()
            host.hh_df_scratch(n, in_dim, nh, rows, F, out)
            pos = 256
            dxg = pos + r256(12 * n)
            part = dxg + r256(4 * in_dim * n)
            acc = part + r256(4 * py_slabs(n) * py_params(in_dim, nh))
            total = acc + r256(8 * rows * F)
            assert list(out) == [pos, dxg, part, acc, total], (n, in_dim, nh)
    assert host.hh_df_weight_offset(10, 1, 0) == 0 and host.hh_df_weight_offset(10, 1, 1) == 176
    assert host.hh_df_weight_offset(14, 2, 1) == 240 and host.hh_df_weight_offset(14, 2, 2) == 240 + 272
    assert host.hh_df_weight_offset(10, 0, 0) == 0


def test_standalone_sanitizer_program(tmp_path):
    """the two headers under -fsanitize=address,undefined as a program of its own: a small net over a few hundred points, edges included"""
    main = tmp_path / "df_main.cpp"
    main.write_text(f'#include "{SRC}"\n' + r'''
#include <cstdio>
#include <vector>
int main() {
    hg::Level lv[3];
    int64_t rows = 0;
    if (hg::levels_tcnn(3, 4, 2.0, 8, lv, &rows)) return 1;
    const int F = 4, in_dim = 12;
    uint32_t seed = 7u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return ((int)(seed >> 8) % 2001 - 1000) / 1000.0f; };
    std::vector<float> table(rows * F), w0(16 * in_dim), w1(256), w2(16), b0(16), b1(16), b2(1), x(3 * 300), h(300), p(3 * 300);
    std::vector<int> sel(300);
    for (auto* v : {&table, &w0, &w1, &w2, &b0, &b1, &b2}) for (auto& e : *v) e = rnd();
    for (auto& e : x) e = 3.0f * rnd();
    x[0] = NAN; x[4] = INFINITY; x[6] = x[7] = x[8] = 0.0f; x[9] = 1.0f;
    const float aabb[6] = {-1, -1, -1, 1, 1, 1};
    for (int nh = 0; nh <= 2; ++nh)
        for (int contraction = 0; contraction <= 1; ++contraction) {
            hh_df_forward(lv, 3, F, table.data(), nh, nh == 0 ? w2.data() : w0.data(), nh == 2 ? w1.data() : w2.data(), w2.data(), b0.data(),
                          b1.data(), b2.data(), nullptr, contraction, aabb, x.data(), 300, h.data(), p.data(), sel.data());
            if (sel[0] != 0 || sel[1] != 0) return 2;        // the NaN and the Inf coordinate
            for (float v : h) if (!(v == v)) return 3;
        }
    int64_t out[5];
    for (int64_t n : {(int64_t)1, (int64_t)65, (int64_t)1 << 24}) hh_df_scratch(n, 64, 2, (int64_t)1 << 24, 8, out);
    std::printf("%lld ok\n", (long long)out[4]);
    return 0;
}
''')
    exe = str(tmp_path / "df_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(main), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok") and "runtime error" not in run.stderr
