"""CPU checks of pixie_amd/csrc/hashgrid_grad_math.h (compiled for the host by tests/host_harness/hashgrid_grad_math_host.cpp, g++
-ffp-contract=off) against Python integers and fractions: the exponent rule of the table gradient's 64-bit fixed-point scatter.

    2^e > M, e minimal;  s = 62 - e - ceil(log2(8 n));  contribution c -> llrint(c 2^s);  accumulator -> float32(double(acc) 2^-s)
"""
import ctypes as C
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "hashgrid_grad_math_host.cpp")
FP = C.POINTER(C.c_float)
N_MAX = 1 << 24


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("hgg_host") / "libhashgrid_grad_math_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_hgg_state.argtypes = [C.c_uint32]
    h.hh_hgg_pow2_above.argtypes = [C.c_uint32]
    h.hh_hgg_shift.argtypes = [C.c_uint32, C.c_int64]
    h.hh_hgg_ceil_log2.argtypes = [C.c_uint64]
    h.hh_hgg_magnitude_bits.argtypes, h.hh_hgg_magnitude_bits.restype = [C.c_float], C.c_uint32
    h.hh_hgg_quantise.argtypes, h.hh_hgg_quantise.restype = [C.c_float, C.c_int], C.c_int64
    h.hh_hgg_finalise.argtypes, h.hh_hgg_finalise.restype = [C.c_int64, C.c_int], C.c_float
    h.hh_hgg_sum.argtypes, h.hh_hgg_sum.restype = [FP, C.c_int64, C.c_int], C.c_int64
    return h


def bits_of(x):
    return int(np.float32(x).view(np.uint32)) & 0x7FFFFFFF


def magnitudes():
    """float32 magnitudes across the range: powers of two and their neighbours, denormals, the extremes, random bit patterns"""
    rng = np.random.default_rng(1)
    out = [np.float32(2.0) ** e for e in range(-126, 128, 7)]
    out += [np.nextafter(v, np.float32(0)) for v in out] + [np.nextafter(v, np.float32(np.inf)) for v in out[:-1]]
    out += [np.uint32(b).view(np.float32) for b in (1, 2, 3, 0x7FFFFF, 0x400000, 0x400001, 0x800000, 0x7F7FFFFF)]
    out += list(rng.integers(1, 0x7F800000, 300, dtype=np.uint32).view(np.float32))
    return [np.float32(v) for v in out]


def test_states_and_magnitude_bits(host):
    assert host.hh_hgg_state(0) == 1
    assert host.hh_hgg_state(bits_of(np.inf)) == 2 and host.hh_hgg_state(bits_of(np.nan)) == 2 and host.hh_hgg_state(0x7FFFFFFF) == 2
    assert host.hh_hgg_state(1) == 0 and host.hh_hgg_state(0x7F7FFFFF) == 0
    for x in (-1.5, 1.5, -0.0, 3e-42, -np.inf):
        assert host.hh_hgg_magnitude_bits(x) == bits_of(abs(np.float32(x)))
    xs = sorted(magnitudes())
    assert [bits_of(x) for x in xs] == sorted(bits_of(x) for x in xs), "the order of the bits is the order of the magnitudes"
    assert bits_of(np.nan) > bits_of(np.inf) > bits_of(xs[-1])


def test_exponent_rule_across_the_float_range(host):
    ns = [1, 2, 3, 4, 5, 63, 64, 65, 1000, 196608, N_MAX - 1, N_MAX]
    for v, want in ((1, 0), (2, 1), (3, 2), (4, 2), (5, 3), (8 * N_MAX, 27), (8 * N_MAX - 1, 27), (2 ** 26 + 1, 27)):
        assert host.hh_hgg_ceil_log2(v) == want
    for m in magnitudes():
        M = Fraction(float(m))
        e = host.hh_hgg_pow2_above(bits_of(m))
        assert Fraction(2) ** (e - 1) <= M < Fraction(2) ** e, (m, e)
        for n in ns:
            s = host.hh_hgg_shift(bits_of(m), n)
            assert s == 62 - e - (8 * n - 1).bit_length(), (m, n)
            # 8 n contributions of magnitude M, all of one sign, stay inside 63 bits
            q = host.hh_hgg_quantise(float(m), s)
            assert q == round(M * Fraction(2) ** s) and 8 * n * q < 2 ** 62 + 8 * n, (m, n, q)
            assert host.hh_hgg_quantise(-float(m), s) == -q
    assert host.hh_hgg_shift(bits_of(1.0), N_MAX) == 62 - 1 - 27 and host.hh_hgg_shift(bits_of(0.999), 1) == 62 - 0 - 3


def test_quantisation_is_exact_up_to_the_integer_rounding(host):
    rng = np.random.default_rng(2)
    for m in (np.float32(1e-30), np.float32(0.37), np.float32(1.0), np.float32(5e20), np.uint32(5).view(np.float32)):
        for n in (1, 200, N_MAX):
            s = host.hh_hgg_shift(bits_of(m), n)
            for c in (rng.uniform(-1, 1, 50).astype(np.float32) * m).astype(np.float32):
                exact = Fraction(float(c)) * Fraction(2) ** s
                q = host.hh_hgg_quantise(float(c), s)
                assert abs(Fraction(q) - exact) <= Fraction(1, 2), (m, n, c)


def test_round_trip_and_order(host):
    rng = np.random.default_rng(3)
    for trial in range(40):
        count = int(rng.integers(1, 2000))
        n = max(count // 8 + 1, int(rng.integers(1, 5000)))
        scale = np.float32(2.0) ** int(rng.integers(-60, 60))
        c = (rng.standard_normal(count) * scale).astype(np.float32)
        if trial % 5 == 0:
            c[rng.integers(0, count, count // 3)] = 0
        m = np.abs(c).max()
        if m == 0:
            continue
        s = host.hh_hgg_shift(bits_of(m), n)
        acc = host.hh_hgg_sum(c.ctypes.data_as(FP), count, s)
        assert acc == sum(host.hh_hgg_quantise(float(v), s) for v in c) and abs(acc) < 2 ** 62
        got = host.hh_hgg_finalise(acc, s)
        exact = math.fsum(float(v) for v in c)
        want = float(np.float32(exact))
        quantum = count * 2.0 ** (-s - 1)
        ulp = float(np.spacing(np.float32(abs(exact) + quantum)))
        assert abs(got - exact) <= quantum + ulp / 2 * (1 + 2.0 ** -20) and abs(got - want) <= quantum + ulp, (trial, got, want, quantum)
        perm = np.ascontiguousarray(c[rng.permutation(count)])
        again = host.hh_hgg_finalise(host.hh_hgg_sum(perm.ctypes.data_as(FP), count, s), s)
        assert np.float32(got).view(np.uint32) == np.float32(again).view(np.uint32), "the order of the list changes the bits"
    assert host.hh_hgg_finalise(0, 40) == 0.0 and host.hh_hgg_finalise(3, 1) == 1.5 and host.hh_hgg_finalise(-3, -2) == -12.0


def test_standalone_sanitizer_program(tmp_path):
    """the header under -fsanitize=address,undefined as a program of its own: shifts, conversions and sums over the same ranges"""
    main = tmp_path / "hgg_main.cpp"
    main.write_text(f'#include "{SRC}"\n' + r'''
#include <cstdio>
#include <cstring>
#include <vector>
int main() {
    uint32_t seed = 12345u;
    long checked = 0;
    for (int e = 1; e < 255; e += 3)
        for (int64_t n : {(int64_t)1, (int64_t)200, (int64_t)1 << 24}) {
            const uint32_t bits = ((uint32_t)e << 23) | (seed & 0x7fffffu);
            float m;
            std::memcpy(&m, &bits, 4);
            const int s = hh_hgg_shift(bits, n);
            std::vector<float> c(64);
            for (auto& v : c) { seed = seed * 1664525u + 1013904223u; v = m * ((int)(seed >> 8) % 2001 - 1000) / 1000.0f; }
            const int64_t acc = hh_hgg_sum(c.data(), (int64_t)c.size(), s);
            if (!(hh_hgg_finalise(acc, s) == hh_hgg_finalise(acc, s))) return 1;
            ++checked;
        }
    for (uint32_t b : {1u, 2u, 0x7fffffu}) if (hh_hgg_shift(b, 1) < 62 + 126 - 3) return 2;
    std::printf("%ld ok\n", checked);
    return 0;
}
''')
    exe = str(tmp_path / "hgg_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           str(main), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok") and "runtime error" not in run.stderr
