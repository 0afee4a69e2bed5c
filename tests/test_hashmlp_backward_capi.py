"""CPU checks of the boundary of the differentiable hash-grid MLP (include/pixie_hip.h, pixie_amd/csrc/field_query_backward.hip): the
entry points are declared, typed and exported, struct pixie_hashmlp_grads is laid out as gcc lays it out, and
pixie_hashmlp_train_bytes returns the documented formula on a host without a device (the pointers below point nowhere and are never
dereferenced)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from pixie_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "pixie_hip.h")
NAMES = ("pixie_hashmlp_train_bytes", "pixie_hashmlp_forward_saved", "pixie_hashmlp_backward")
FAKE = 1 << 20


def desc(n_levels=4, F=2, n_freq=0, n_extra=0, n_hidden=2, out_dim=80, rows=1000):
    d = _lib.HashMlpDesc()
    d.n_levels, d.features_per_level, d.n_frequencies, d.n_extra, d.n_hidden, d.out_dim = n_levels, F, n_freq, n_extra, n_hidden, out_dim
    for l in range(n_levels):
        d.level[l].scale, d.level[l].shift, d.level[l].res, d.level[l].size, d.level[l].offset = 3.0 * (l + 1), 0.5, 4 * (l + 1), rows // n_levels, l * (rows // n_levels)
    d.d_table, d.table_rows = (FAKE if n_levels else None), (rows if n_levels else 0)
    for i in range(n_hidden + 1):
        d.d_weight[i] = FAKE
    return d


def test_declared_typed_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    prod = text.partition("#ifdef PIXIE_DIAG")[0]
    assert re.search(r"\}\s*pixie_hashmlp_grads\s*;", prod)
    syms = lambda p: {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", p], text=True).splitlines()}
    for nm in NAMES:
        assert re.search(r"\b" + nm + r"\s*\(", prod), nm
        assert nm in _lib.SIGNATURES and nm not in _lib.DIAG_SIGNATURES
        assert nm in syms(_lib.LIB_PATH) and nm in syms(_lib.DIAG_LIB_PATH)
    D, G, VP, I64 = C.POINTER(_lib.HashMlpDesc), C.POINTER(_lib.HashMlpGrads), C.c_void_p, C.c_int64
    assert _lib.SIGNATURES["pixie_hashmlp_train_bytes"] == (C.c_int, [D, I64, C.POINTER(I64), C.POINTER(I64)])
    assert _lib.SIGNATURES["pixie_hashmlp_forward_saved"] == (C.c_int, [D, VP, VP, I64, VP, VP, VP])
    assert _lib.SIGNATURES["pixie_hashmlp_backward"] == (C.c_int, [D, VP, VP, I64, VP, VP, VP, G, VP, VP])


def test_grads_layout_matches_header(tmp_path):
    cls, cname = _lib.HashMlpGrads, "pixie_hashmlp_grads"
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {", f'printf("sizeof %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "hashmlp_grads_layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    exe = tmp_path / "hashmlp_grads_layout"
    subprocess.check_call(["gcc", "-std=c99", "-o", str(exe), str(src)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["sizeof"]) == C.sizeof(cls) == 8 * (2 + 2 * _lib.HASHMLP_MAX_LAYERS)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


def documented_bytes(d, n):
    """the formula of include/pixie_hip.h, restated"""
    F = d.features_per_level if d.n_levels else 0
    in_dim = d.n_levels * F + 6 * d.n_frequencies + d.n_extra
    up = lambda b: -(-b // 256) * 256
    tiles = -(-n // 64)
    shapes = [(64, in_dim)] + [(64, 64)] * (d.n_hidden - 1) + [(d.out_dim, 64)]
    slabs = lambda o, k: max(1, min(1024 // (-(-o // 64) * -(-k // 64)), 256, tiles))
    part = max(slabs(o, k) * (o * k + o) for o, k in shapes)
    scratch = 256 + up(4 * 64 * d.n_hidden * n) + up(4 * d.n_levels * F * n) + up(4 * part) + up(8 * d.table_rows * F)
    return 4 * n * (in_dim + 64 * d.n_hidden), scratch


@pytest.mark.parametrize("kw", [dict(), dict(F=8, n_freq=6, out_dim=768, n_levels=12, rows=24000), dict(n_levels=0, F=0, n_extra=15, out_dim=3),
                                dict(n_extra=15, n_hidden=4, out_dim=1), dict(F=4, n_hidden=1)])
@pytest.mark.parametrize("n", [0, 1, 64, 65, 200, 196608, 1 << 24])
def test_train_bytes_is_the_documented_formula(kw, n):
    lib, d = _lib.load(), desc(**kw)
    saved, scratch = C.c_int64(-1), C.c_int64(-1)
    assert lib.pixie_hashmlp_train_bytes(C.byref(d), n, C.byref(saved), C.byref(scratch)) == 0, lib.pixie_last_error()
    assert (saved.value, scratch.value) == documented_bytes(d, n)
    assert lib.pixie_hashmlp_train_bytes(C.byref(d), n, None, None) == 0


def test_refusals_need_no_device():
    lib, d = _lib.load(), desc()
    for fn, args in ((lib.pixie_hashmlp_train_bytes, (None, None)), (lib.pixie_hashmlp_forward_saved, (None, None, None, None)),):
        assert fn(C.byref(d), *([None, None] if fn is lib.pixie_hashmlp_forward_saved else []), (1 << 24) + 1, *args) != 0
        assert b"2^24" in lib.pixie_last_error()
    g = _lib.HashMlpGrads()
    assert lib.pixie_hashmlp_backward(C.byref(d), None, None, (1 << 24) + 1, None, None, None, C.byref(g), None, None) != 0 and b"2^24" in lib.pixie_last_error()
    assert lib.pixie_hashmlp_backward(C.byref(d), FAKE, None, 10, FAKE, FAKE, FAKE, None, FAKE, None) != 0 and b"grads" in lib.pixie_last_error()
    assert lib.pixie_hashmlp_backward(C.byref(d), FAKE, None, 10, FAKE, FAKE, FAKE, C.byref(g), None, None) == 0, "no gradient asked for: a no-op"
    g.d_extra = FAKE
    assert lib.pixie_hashmlp_backward(C.byref(d), FAKE, None, 10, FAKE, FAKE, FAKE, C.byref(g), FAKE, None) != 0 and b"d_extra" in lib.pixie_last_error()
    g = _lib.HashMlpGrads()
    g.d_weight[0] = FAKE
    assert lib.pixie_hashmlp_backward(C.byref(d), FAKE, None, 10, FAKE, FAKE, FAKE, C.byref(g), None, None) != 0 and b"d_scratch" in lib.pixie_last_error()
    assert lib.pixie_hashmlp_backward(C.byref(d), FAKE, None, 10, FAKE, FAKE, FAKE, C.byref(g), FAKE + 16, None) != 0 and b"256" in lib.pixie_last_error()
    g.d_weight[4] = FAKE
    assert lib.pixie_hashmlp_backward(C.byref(d), FAKE, None, 10, FAKE, FAKE, FAKE, C.byref(g), FAKE, None) != 0 and b"layer 4" in lib.pixie_last_error()
    bad = desc()
    bad.n_hidden = 5
    assert lib.pixie_hashmlp_train_bytes(C.byref(bad), 10, None, None) != 0 and b"hidden" in lib.pixie_last_error()
    assert lib.pixie_hashmlp_forward_saved(C.byref(d), FAKE, None, 10, FAKE, None, None) != 0 and b"d_saved" in lib.pixie_last_error()
