"""CPU checks of pixie_amd/csrc/hashgrid_math.h (compiled for the host by tests/host_harness/hashgrid_math_host.cpp, g++
-ffp-contract=off) against the NumPy restatement of tests/_field_query_ref.py, and of the Python side of pixie_amd/field_query.py
that needs no device: level tables, the tiny-cuda-nn parameter split, the colour-head fold, spherical harmonics.

Equalities: level tables (scale, shift, res, size, offset, dense, total), lattice coordinates (also against torch.arange), unit
positions and selectors, corner rows.  The float32 blend of the header against the float64 restatement: 8 products and 7 sums per
column, each within one rounding, so |err| <= 16 2^-24 max|table|.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from pixie_amd import _lib, field_query as FQ
from tests import _field_query_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "hashgrid_math_host.cpp")
CONFIGS = [(4, 4, 32, 8), (12, 16, 128, 19), (16, 16, 2048, 19)]
FP, U32, I32 = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("hg_host") / "libhashgrid_math_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_hg_levels.argtypes = [C.c_int] * 5 + [C.POINTER(_lib.HashGridLevel), C.POINTER(C.c_int64)]
    h.hh_hg_lattice.argtypes = [C.c_double, C.c_double, C.c_int, FP]
    h.hh_hg_unit.argtypes = [FP, C.c_int, FP, FP, C.c_int64, FP, I32]
    h.hh_hg_unit_position.argtypes = [FP, C.c_int, FP, FP, C.c_int64, FP, I32]
    h.hh_hg_corners.argtypes = [C.POINTER(_lib.HashGridLevel), FP, C.c_int64, U32, FP]
    h.hh_hg_encode.argtypes = [C.POINTER(_lib.HashGridLevel), C.c_int, FP, C.c_int, FP, C.c_int64, FP]
    h.hh_hg_frequency_args.argtypes = [FP, C.c_int64, C.c_int, FP]
    return h


def fp(a):
    return a.ctypes.data_as(FP)


def host_levels(h, convention, cfg):
    lv = (_lib.HashGridLevel * 16)()
    total = C.c_int64()
    assert h.hh_hg_levels(0 if convention == "nerfstudio" else 1, *cfg, lv, C.byref(total)) == 0
    return lv, total.value


def points(rng, n):
    p = rng.random((n, 3)).astype(np.float32)
    p[:6] = [[0, 0, 0], [1, 1, 1], [0.5, 0.25, 0.75], [0, 1, 0.5], [0.125, 0.125, 0.125], [1, 0, 0]]     # 0, 1 and cell boundaries
    return p


@pytest.mark.parametrize("convention", ["nerfstudio", "tcnn"])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_level_tables_of_header_python_and_restatement_agree(host, convention, cfg):
    lv, total = host_levels(host, convention, cfg)
    ref, ref_total = R.levels(convention, *cfg)
    py, py_total = (FQ.nerfstudio_levels(*cfg) if convention == "nerfstudio" else
                    FQ.tcnn_levels(cfg[0], cfg[1], FQ.growth_factor(cfg[0], cfg[1], cfg[2]), cfg[3]))
    assert total == ref_total == py_total
    T = 2 ** cfg[3]
    for l, r in enumerate(ref):
        got = {k: getattr(lv[l], k) for k in ("scale", "shift", "size", "offset", "dense")}
        assert got == {k: r[k] for k in got}, (l, got, r)
        assert {k: py[l][k] for k in got} == {k: r[k] for k in got}, l
        if convention == "tcnn":
            assert lv[l].res == r["res"] == py[l]["res"]
    if convention == "nerfstudio":
        assert all(r["dense"] == 0 and r["size"] == T and r["offset"] == l * T for l, r in enumerate(ref)) and total == cfg[0] * T
        # the module's own expression, evaluated by torch as the module evaluates it
        want = torch.floor(cfg[1] * R.growth(*cfg[:3]) ** torch.arange(cfg[0]))
        assert [r["scale"] for r in ref] == want.tolist()
    else:
        dense = [r["dense"] for r in ref]
        switch = dense.index(0) if 0 in dense else len(dense)
        assert dense == [1] * switch + [0] * (len(dense) - switch), "dense levels come first"
        assert all((r["res"] ** 3 <= T) == bool(r["dense"]) for r in ref)
        assert all(r["size"] == min(-(-r["res"] ** 3 // 8) * 8, T) and r["size"] % 8 == 0 for r in ref)
        assert [r["offset"] for r in ref] == np.concatenate([[0], np.cumsum([r["size"] for r in ref])[:-1]]).tolist()
        assert total == sum(r["size"] for r in ref)
    if cfg == (4, 4, 32, 8) and convention == "tcnn":
        assert dense == [1, 0, 0, 0] and [r["res"] for r in ref] == [4, 8, 16, 32]
    if cfg == (16, 16, 2048, 19) and convention == "nerfstudio":
        assert ref[-1]["scale"] == 2047.0, "float32 power: the last level falls one short of max_res"


@pytest.mark.parametrize("lo,step,n,exact", [(-0.5, 0.01, 100, False), (-0.5, 1.0 / 16, 16, True), (-0.37, 0.0625 * 1.1, 16, False), (0.1, 0.3, 5, True)])
def test_lattice_coordinate_against_torch_arange(host, lo, step, n, exact):
    """The closed form float32(double(min) + i double(step)) equals the restatement always, and torch.arange on the CPU where the
    vector loop of arange does not round differently: steps that are exact in float32, and runs shorter than a vector (the scalar
    tail computes in double).  Elsewhere arange fills its lanes as float32(base) + float32(step) k and lands within a few ulps of
    the step; which elements differ depends on the CPU's vector width, so FeatureFieldQuery.voxelize does not use the closed form
    but hands the kernel torch.arange's own output (lattice_axes)."""
    out = np.zeros(n, np.float32)
    host.hh_hg_lattice(lo, step, n, fp(out))
    assert np.array_equal(out, R.lattice((lo, lo, lo), step, (n, 1, 1))[:, 0, 0, 0])
    hi = lo + step * n - step / 2
    want = torch.arange(lo, hi, step)
    assert len(want) == n
    if exact:
        assert np.array_equal(out, want.numpy())
    else:
        assert np.abs(out.astype(np.float64) - want.numpy()).max() <= 4 * 2.0 ** -24 * max(abs(lo), abs(hi))
    axes = FQ.lattice_axes((lo,) * 3, (hi,) * 3, step)
    assert all(torch.equal(a, want) and a.dtype == torch.float32 for a in axes)


@pytest.mark.parametrize("contraction", [True, False])
def test_unit_positions_and_selector_equal_the_restatement(host, contraction):
    rng = np.random.default_rng(3)
    x = (rng.random((4000, 3)) * 5 - 2.5).astype(np.float32)
    x[:5] = [[1, 0.5, -0.5], [-1, -1, 1], [0, 0, 0], [2, -3, 0.5], [0.999999, 0, 0]]        # |x|_inf exactly 1, above, below
    A = np.array([[0.9, 0.1, 0, 0.05], [-0.1, 0.9, 0, 0], [0, 0, 1.1, -0.02]], np.float32)
    aabb = np.array([[-1, -1.5, -1], [1, 1, 2]], np.float32)
    for M in (np.eye(4, dtype=np.float32)[:3], A):
        p, sel = np.zeros_like(x), np.zeros(len(x), np.int32)
        host.hh_hg_unit(fp(np.ascontiguousarray(M)), int(contraction), fp(aabb), fp(x), len(x), fp(p), sel.ctypes.data_as(I32))
        want_p, want_sel = R.world_to_unit(x, M, contraction, aabb)
        assert np.array_equal(p.view(np.uint32), want_p.view(np.uint32))
        assert np.array_equal(sel.astype(bool), want_sel)
        assert sel.all() if contraction else 0 < sel.sum() < len(x)      # every finite point contracts to the inside of the cube
    # hg::unit_position itself, the function the kernels call: with the affine, and without one (null), where the restatement's
    # identity affine is exact for finite coordinates
    x[5:8] = [[np.nan, 0.25, 0.5], [-1, 1, -1], [3, 0.5, 2.5]]                  # a NaN coordinate, |x|_inf exactly 1, a point outside
    finite = np.arange(len(x)) != 5
    for M in (None, A):
        p, sel = np.zeros_like(x), np.zeros(len(x), np.int32)
        host.hh_hg_unit_position(fp(M) if M is not None else None, int(contraction), fp(aabb), fp(x), len(x), fp(p), sel.ctypes.data_as(I32))
        want_p, want_sel = R.world_to_unit(x[finite], np.eye(4, dtype=np.float32)[:3] if M is None else M, contraction, aabb)
        assert np.array_equal(p[finite].view(np.uint32), want_p.view(np.uint32))
        assert np.array_equal(sel[finite].astype(bool), want_sel)
        assert sel[5] == 0 and np.isnan(p[5, 0]), "a NaN coordinate stays NaN and selects nothing"
        assert sel[7] == int(contraction), "a point outside: contracted into the cube, or left outside the aabb"
        if M is None:
            want6 = [0.25, 0.75, 0.25] if contraction else [0, 1, 0]           # the far branch of the contraction is the identity at 1
            assert np.array_equal(p[6], np.float32(want6)) and sel[6] == int(contraction)


@pytest.mark.parametrize("convention", ["nerfstudio", "tcnn"])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_corner_rows_and_blend_equal_the_restatement(host, convention, cfg):
    rng = np.random.default_rng(5)
    lv, total = host_levels(host, convention, cfg)
    ref, _ = R.levels(convention, *cfg)
    p = points(rng, 500)
    F = 2
    table = rng.uniform(-1, 1, (total, F)).astype(np.float32)
    out = np.zeros((len(p), cfg[0] * F), np.float32)
    host.hh_hg_encode(lv, cfg[0], fp(table), F, fp(p), len(p), fp(out))
    want = R.encode(ref, table, p)
    err = np.abs(out - want).max()
    print(f"{convention} {cfg}: |blend - float64| {err:.3e}, bar {16 * 2.0 ** -24:.3e}")
    assert err <= 16 * 2.0 ** -24
    for l in (0, cfg[0] - 1):
        rows, w = np.zeros((len(p), 8), np.uint32), np.zeros((len(p), 8), np.float32)
        host.hh_hg_corners(C.byref(lv[l]), fp(p), len(p), rows.ctypes.data_as(U32), fp(w))
        assert rows.min() >= ref[l]["offset"] and rows.max() < ref[l]["offset"] + ref[l]["size"]
        assert np.allclose(w.sum(axis=1), 1.0, atol=4e-7) and w.min() >= 0
    if convention == "nerfstudio":
        lit = R.encode_nerfstudio([r["scale"] for r in ref], cfg[3], table, p)
        assert np.abs(lit - want).max() <= 16 * 2.0 ** -53 * 4, "ceil / floor form and floor / floor + 1 form of the same grid"


def test_frequency_arguments(host):
    rng = np.random.default_rng(7)
    p = points(rng, 64)
    out = np.zeros((64, 36), np.float32)
    host.hh_hg_frequency_args(fp(p), 64, 6, fp(out))
    want = R.frequency(p, 6)
    got = np.where(np.arange(36) % 2 == 1, np.cos(out.astype(np.float64)), np.sin(out.astype(np.float64)))
    assert np.abs(got - want).max() <= 32 * np.pi * 2.0 ** -23         # one rounding of an argument of at most 32 pi


def test_standalone_sanitizer_program(tmp_path):
    """the same cases under -fsanitize=address,undefined as a program of its own: tables hold exactly the rows the level tables
    claim, so a corner row out of range is a reported heap overflow"""
    exe = str(tmp_path / "hashgrid_math_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DHG_STANDALONE", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith("ok") and "runtime error" not in run.stderr


def test_descriptor_layouts_match_the_header(tmp_path):
    header = os.path.join(os.path.dirname(HERE), "include", "pixie_hip.h")
    structs = {"pixie_hashgrid_level": _lib.HashGridLevel, "pixie_hashmlp_desc": _lib.HashMlpDesc, "pixie_field_voxelize_desc": _lib.FieldVoxelizeDesc}
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{header}"', "int main(void) {",
             'printf("consts %d %d %d %d\\n", PIXIE_HASHMLP_MAX_LEVELS, PIXIE_HASHMLP_MAX_LAYERS, PIXIE_HASHMLP_MAX_INPUT, PIXIE_HASHMLP_MAX_OUTPUT);']
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]))
    subprocess.check_call(["gcc", "-std=c99", "-o", str(tmp_path / "layout"), str(src)])
    rows = [l.split() for l in subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines()]
    assert [int(v) for v in rows[0][1:]] == [_lib.HASHMLP_MAX_LEVELS, _lib.HASHMLP_MAX_LAYERS, _lib.HASHMLP_MAX_INPUT, _lib.HASHMLP_MAX_OUTPUT]
    got = {r[0]: int(r[1]) for r in rows[1:]}
    for cname, cls in structs.items():
        assert got[cname] == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert got[f"{cname}.{f}"] == getattr(cls, f).offset, f"{cname}.{f}"


def test_sh_closed_forms_and_color_fold():
    rng = np.random.default_rng(11)
    for d in ([0.5, 0.5, 0.5], [0, 0, 0], [0.3, -0.2, 0.9]):
        assert np.allclose(FQ.sh_components(4, d), R.sh(4, d), rtol=1e-14, atol=1e-15)
    assert FQ.sh_components(2, [0, 0, 1]).shape == (4,)
    w = [rng.standard_normal((64, 16 + 15 + 8)), rng.standard_normal((64, 64)), rng.standard_normal((3, 64))]
    b = [rng.standard_normal(64), None, rng.standard_normal(3)]
    dirs, app, geo = R.sh(4, [0.5, 0.5, 0.5]), rng.standard_normal(8), rng.standard_normal((10, 15))
    fw, fb = FQ.fold_color_head(w, b, 16, 15, dirs, app)
    full = np.concatenate([np.tile(dirs, (10, 1)), geo, np.tile(app, (10, 1))], axis=1)
    assert np.allclose(R.mlp(geo, fw, fb, "sigmoid"), R.mlp(full, w, b, "sigmoid"), atol=2e-6)
    with pytest.raises(ValueError):
        FQ.fold_color_head(w, b, 16, 14, dirs, app)


def test_tcnn_parameter_split_and_its_refusals():
    rng = np.random.default_rng(13)
    lv, rows = FQ.tcnn_levels(4, 4, FQ.growth_factor(4, 4, 32), 8)
    in_dim, out_dim, F = 4 * 8 + 36, 20, 8                       # 68 columns -> padded to 80, 20 outputs -> padded to 32
    w0, w1, w2 = rng.standard_normal((64, 80)), rng.standard_normal((64, 64)), rng.standard_normal((32, 64))
    table = rng.standard_normal((rows, F))
    params = np.concatenate([w0.ravel(), w1.ravel(), w2.ravel(), table.ravel()]).astype(np.float32)
    ws, bs, t = FQ.split_tcnn_params(params, in_dim, 2, out_dim, rows, F)
    assert [w.shape for w in ws] == [(64, 68), (64, 64), (20, 64)] and t.shape == (rows, F)
    assert np.array_equal(ws[0], w0[:, :68].astype(np.float32)) and np.array_equal(ws[2], w2[:20].astype(np.float32))
    assert np.array_equal(t, table.astype(np.float32)) and bs[1] is None and bs[2] is None
    assert np.allclose(bs[0], w0[:, 68:].sum(axis=1), atol=1e-5), "padding columns hold 1.0: their weights sum into a bias"
    for bad in (params[:-1], np.concatenate([params, [0.0]])):
        with pytest.raises(ValueError, match="parameters"):
            FQ.split_tcnn_params(bad, in_dim, 2, out_dim, rows, F)
    ws, bs, t = FQ.split_tcnn_params(np.zeros(64 * 32 + 16 * 64, np.float32), 32, 1, 16)
    assert bs == [None, None] and t is None


def test_host_side_refusals_need_no_device():
    with pytest.raises(ValueError):
        FQ.nerfstudio_levels(17, 16, 2048, 19)
    with pytest.raises(ValueError):
        FQ.tcnn_levels(4, 4, 2.0, 25)
    with pytest.raises(_lib.PixieHipError):
        FQ.HashMLP(None, None, [np.zeros((64, 3)), np.zeros((3, 64))], n_extra=3, device="cpu")
