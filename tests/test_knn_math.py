"""CPU checks of pixie_amd/csrc/knn_math.h (compiled for the host by tests/host_harness/knn_math_host.cpp, g++ -ffp-contract=off):
the arithmetic of distCUDA2, through the same Morton, box and pruning path as the kernels of knn.hip, against the two references
of tests/_knn_ref.py.

Bars.  The header's result is BIT-EQUAL to brute32 (same float32 expression order; the search is exact).  brute32 itself lies
within 8 * 2^-24 relative of brute64: a coordinate difference carries u = 2^-24, its square and the three-term sum 5 u, the sum of
three distances and the division 3 u.

Fewer than four points.  A missing neighbour counts as FLT_MAX, as in simple-knn.  One or two points therefore give +inf (FLT_MAX +
FLT_MAX overflows).  Three points do NOT: (b0 + b1) + FLT_MAX rounds back to FLT_MAX unless b0 + b1 reaches 2^103, so the value is
FLT_MAX / 3 = 1.1342745e38 -- which is also what the reference's kernel returns; the test pins that, and that no value is small."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import _knn_ref as kr

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "knn_math_host.cpp")
FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("knn_host") / "libknn_math_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_knn_morton.argtypes = [C.c_int, FP, FP, FP, C.POINTER(C.c_uint32)]
    h.hh_knn_mean_dist2.argtypes = [C.c_int, FP, C.c_int, FP, C.POINTER(C.c_int64)]
    return h


def host_knn(h, p, group):
    p = np.ascontiguousarray(p, np.float32)
    out = np.full((len(p),), np.nan, np.float32)
    visited = C.c_int64(0)
    assert h.hh_knn_mean_dist2(len(p), p.ctypes.data_as(FP), group, out.ctypes.data_as(FP), C.byref(visited)) == 0
    return out, visited.value


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


CASES = [("uniform2500", lambda: kr.uniform(2500, 10))] + list(kr.CLOUDS.items())


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("group", [8, 64])
def test_header_is_bit_equal_to_the_float32_brute_force(host, name, make, group):
    p = make()
    ref = kr.brute32(p)
    got, visited = host_knn(host, p, group)
    assert np.array_equal(bits(got), bits(ref)), f"{name}: {int((bits(got) != bits(ref)).sum())} of {len(p)} differ"
    print(f"{name}, boxes of {group}: {visited / len(p):.0f} distances per point of {len(p) - 1}")
    if name in ("uniform2500", "clustered", "planar") and group == 8:
        assert visited < 0.5 * len(p) * (len(p) - 1), "no pruning took place"


@pytest.mark.parametrize("name,make", [c for c in CASES if c[0] in ("uniform2500", "clustered", "planar")],
                         ids=["uniform2500", "clustered", "planar"])
def test_float32_brute_force_against_float64(name, make):
    p = make()
    r32, r64 = kr.brute32(p).astype(np.float64), kr.brute64(p)
    rel = np.max(np.abs(r32 - r64) / r64)
    print(f"{name}: brute32 against brute64, worst relative error {rel / 2.0 ** -24:.2f} u")
    assert rel <= 8 * 2.0 ** -24


def test_permutation_gives_the_permuted_result(host):
    p = kr.clustered()
    perm = np.random.default_rng(5).permutation(len(p))
    a, _ = host_knn(host, p, 8)
    b, _ = host_knn(host, p[perm], 8)
    assert np.array_equal(bits(a[perm]), bits(b))


def test_fewer_than_four_points(host):
    for n in (1, 2, 3):
        p = kr.uniform(n, 20 + n)
        got, _ = host_knn(host, p, 8)
        ref = kr.brute32(p)
        assert np.array_equal(bits(got), bits(ref))
        if n <= 2:
            assert np.all(np.isposinf(got)), (n, got)
        else:
            assert np.array_equal(bits(got), bits(np.full(3, kr.FLT_MAX / np.float32(3.0), np.float32))), got
    got, _ = host_knn(host, kr.uniform(4, 30), 8)
    assert np.all(np.isfinite(got)) and np.all(got < 12.0)


def test_morton_code_of_a_zero_extent_axis_and_the_corners(host):
    lo, hi = np.array([0.0, -1.0, 2.0], np.float32), np.array([1.0, 1.0, 2.0], np.float32)
    p = np.array([[0.0, -1.0, 2.0], [1.0, 1.0, 2.0], [1.0, -1.0, 2.0], [0.5, 0.0, 2.0]], np.float32)
    codes = np.zeros(4, np.uint32)
    host.hh_knn_morton(4, p.ctypes.data_as(FP), lo.ctypes.data_as(FP), hi.ctypes.data_as(FP), codes.ctypes.data_as(C.POINTER(C.c_uint32)))

    def spread(v):
        return sum(((v >> k) & 1) << (3 * k) for k in range(10))
    assert codes[0] == 0
    assert codes[1] == spread(1023) | (spread(1023) << 1)           # z has no extent: cell 0, no division by zero
    assert codes[2] == spread(1023)
    assert codes[3] == spread(511) | (spread(511) << 1)
    assert int(codes.max()) < 1 << 30
