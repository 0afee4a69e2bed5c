"""CPU checks of the density field's C boundary (include/pixie_hip.h, pixie_amd/csrc/density_field.hip): every malformed descriptor is
refused with a message before any device call (this process has no device to call), and the byte queries agree with the layout the
header documents."""
import ctypes as C

import pytest

from pixie_amd import _lib
from pixie_amd._lib import DensityFieldDesc, DensityFieldGrads

FAKE = 0x10000          # a 16-byte aligned address nobody reads: refusals come before any launch


def good(n_levels=5, F=2, n_hidden=1, log2_T=12):
    d = DensityFieldDesc()
    d.n_levels, d.features_per_level, d.n_hidden, d.hidden_width, d.contraction, d.average_init_density = n_levels, F, n_hidden, 16, 1, 1.0
    T = 1 << log2_T
    for l in range(n_levels):
        d.level[l].scale, d.level[l].shift, d.level[l].res, d.level[l].size, d.level[l].offset, d.level[l].dense = 16.0 * 2 ** l, 0.0, 16 * 2 ** l + 1, T, l * T, 0
    d.d_table, d.table_rows = FAKE, n_levels * T
    for i in range(n_hidden + 1):
        d.d_weight[i] = FAKE
    d.aabb = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
    return d


def edit(**kw):
    d = good()
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def no_contraction_empty_box():
    d = edit(contraction=0)
    d.aabb = (C.c_float * 6)(-1, -1, -1, 1, -1, 1)        # hi == lo on y
    return d


def seventeen_levels():
    d = good()
    d.n_levels = 17
    return d


def weight_missing():
    d = good(n_hidden=2)
    d.d_weight[1] = None
    return d


MALFORMED = {
    "width 64": (lambda: edit(hidden_width=64), b"hidden_width 64 is not 16"),
    "F = 3": (lambda: edit(features_per_level=3), b"features_per_level 3"),
    "17 levels": (seventeen_levels, b"n_levels 17"),
    "table too short": (lambda: edit(table_rows=5 * 4096 - 1), b"does not fit the table"),
    "n_hidden = 3": (lambda: edit(n_hidden=3), b"3 hidden layers"),
    "empty aabb without contraction": (no_contraction_empty_box, b"empty aabb"),
    "input row too wide": (lambda: good(n_levels=16, F=8), b"input row of 128 columns"),
    "null table": (lambda: edit(d_table=None), b"d_table is null"),
    "misaligned table": (lambda: edit(d_table=FAKE + 4), b"16-byte aligned"),
    "missing weight": (weight_missing, b"d_weight[1] is null"),
}


@pytest.mark.parametrize("what", sorted(MALFORMED))
def test_malformed_descriptor_is_refused_by_every_entry_point(what):
    lib = _lib.load()
    make, message = MALFORMED[what]
    d = make()
    saved, scratch = C.c_int64(-1), C.c_int64(-1)
    g = DensityFieldGrads()
    g.d_table = FAKE
    for call in (lambda: lib.pixie_density_field_train_bytes(C.byref(d), 1024, C.byref(saved), C.byref(scratch)),
                 lambda: lib.pixie_density_field_forward(C.byref(d), FAKE, 1024, FAKE, None, None),
                 lambda: lib.pixie_density_field_backward(C.byref(d), FAKE, 1024, FAKE, C.byref(g), FAKE, None)):
        assert call() != 0
        assert message in lib.pixie_last_error(), lib.pixie_last_error()
    assert saved.value == -1 and scratch.value == -1


def test_too_many_points_and_null_arguments():
    lib = _lib.load()
    d = good()
    assert lib.pixie_density_field_train_bytes(C.byref(d), (1 << 24) + 1, None, None) != 0 and b"2^24" in lib.pixie_last_error()
    assert lib.pixie_density_field_forward(C.byref(d), FAKE, (1 << 24) + 1, FAKE, None, None) != 0 and b"2^24" in lib.pixie_last_error()
    assert lib.pixie_density_field_forward(C.byref(d), FAKE, -1, FAKE, None, None) != 0
    assert lib.pixie_density_field_forward(None, FAKE, 1, FAKE, None, None) != 0 and b"null descriptor" in lib.pixie_last_error()
    assert lib.pixie_density_field_forward(C.byref(d), None, 16, FAKE, None, None) != 0 and b"is null" in lib.pixie_last_error()
    assert lib.pixie_density_field_backward(C.byref(d), FAKE, 16, FAKE, None, FAKE, None) != 0 and b"grads is null" in lib.pixie_last_error()
    g = DensityFieldGrads()
    g.d_weight[2] = FAKE                                   # a network of two layers has no third gradient
    assert lib.pixie_density_field_backward(C.byref(d), FAKE, 16, FAKE, C.byref(g), FAKE, None) != 0 and b"layer 2 of 2" in lib.pixie_last_error()
    g = DensityFieldGrads()
    g.d_table = FAKE
    assert lib.pixie_density_field_backward(C.byref(d), FAKE, 16, FAKE, C.byref(g), FAKE + 16, None) != 0 and b"256-byte aligned" in lib.pixie_last_error()
    assert lib.pixie_density_field_backward(C.byref(d), FAKE, 16, FAKE, C.byref(DensityFieldGrads()), None, None) == 0, "no gradient wanted: nothing to do"
    assert lib.pixie_density_field_forward(C.byref(d), None, 0, None, None, None) == 0, "n = 0 is the empty call"


@pytest.mark.parametrize("n", [1, 64, 65, 1 << 20, 1 << 24])
@pytest.mark.parametrize("shape", [(5, 2, 1, 12), (7, 2, 2, 10), (3, 4, 1, 8), (5, 2, 0, 12)])
def test_byte_queries(n, shape):
    lib = _lib.load()
    L, F, nh, T = shape
    d = good(L, F, nh, T)
    saved, scratch = C.c_int64(-1), C.c_int64(-1)
    assert lib.pixie_density_field_train_bytes(C.byref(d), n, C.byref(saved), C.byref(scratch)) == 0
    in_dim, rows = L * F, L << T
    params = in_dim + 1 if nh == 0 else 16 * in_dim + 16 + (nh - 1) * 272 + 17
    slabs = max(1, min(-(-n // 256), 1024))
    r256 = lambda b: -(-b // 256) * 256
    assert saved.value == 0, "the backward recomputes the forward"
    assert scratch.value == 256 + r256(12 * n) + r256(4 * in_dim * n) + r256(4 * slabs * params) + r256(8 * rows * F)
    assert lib.pixie_density_field_train_bytes(C.byref(d), n, None, None) == 0
