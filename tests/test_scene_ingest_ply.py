"""CPU checks of the checkpoint loader of pixie_amd/scene_ingest.py: header parsing, the column table, the refusals, the directory
rule of load_checkpoint, and generate_rotation_matrices against tests/golden/scene_ingest.npz."""
import os

import numpy as np
import pytest
import torch

from pixie_amd import scene_ingest as si
from pixie_amd.ply_io import write_ply, write_ply_f4
from pixie_amd.splat_export import attribute_names, write_vertex_block
from tests import _ingest_ref as ir


def fields(ck):
    """(xyz, raw opacity, log-scales, quaternions, shs (N, K, 3)) read through the column table on the host"""
    b, c, k = ck.block, ck.columns, ck.n_sh_coeffs
    shs = np.concatenate([b[:, c[11:14]][:, None, :], b[:, c[14:11 + 3 * k]].reshape(len(ck), 3, k - 1).transpose(0, 2, 1)], axis=1)
    return b[:, c[0:3]], b[:, c[3:4]], b[:, c[4:7]], b[:, c[7:11]], shs


@pytest.mark.parametrize("case", ["deg0", "deg3"])
def test_reads_the_golden_checkpoints(case):
    cfg = ir.golden_config(case)
    ck = si.load_gaussian_ply(ir.golden_ply(case), cfg["sh_degree"])
    f32 = ir.golden_runs(case)[0]
    xyz, raw, ls, q, shs = fields(ck)
    assert ck.max_sh_degree == ck.active_sh_degree == cfg["sh_degree"] and len(ck) == len(f32["all_xyz"])
    assert np.array_equal(xyz, f32["all_xyz"]) and np.array_equal(shs, f32["all_shs"])      # get_xyz, get_features of the reference


def test_permuted_and_extra_columns_give_the_same_table_view(tmp_path):
    ck = si.load_gaussian_ply(ir.golden_ply("deg3"), 3)
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(ck.names))
    names = [ck.names[i] for i in perm] + ["confidence"]
    block = np.concatenate([ck.block[:, perm], rng.normal(size=(len(ck), 1)).astype(np.float32)], axis=1)
    path = str(tmp_path / "permuted.ply")
    write_ply_f4(path, names, block)
    other = si.load_gaussian_ply(path, 3)
    assert not np.array_equal(other.columns, ck.columns)
    for a, b in zip(fields(ck), fields(other)):
        assert np.array_equal(a, b)


def test_reads_back_what_splat_export_writes(tmp_path):
    rng = np.random.default_rng(1)
    n, k = 17, 4
    block = rng.normal(size=(n, len(attribute_names(k)))).astype(np.float32)
    path = write_vertex_block(str(tmp_path / "frames" / "frame_00000.ply"), torch.from_numpy(block), attribute_names(k))
    ck = si.load_gaussian_ply(path, 1)
    assert ck.names == attribute_names(k) and np.array_equal(ck.block, block)
    assert list(ck.columns[:11]) == [ck.names.index(n_) for n_ in ["x", "y", "z", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]]


def test_every_refusal(tmp_path):
    names = attribute_names(4)
    block = np.zeros((3, len(names)), np.float32)
    good = str(tmp_path / "good.ply")
    write_ply_f4(good, names, block)
    si.load_gaussian_ply(good, 1)
    with pytest.raises(ValueError, match="f_rest"):          # the reference's assert
        si.load_gaussian_ply(good, 3)
    with pytest.raises(ValueError, match="f_rest"):
        si.load_gaussian_ply(good, 0)
    keep = [i for i, n in enumerate(names) if n != "rot_2"]
    missing = str(tmp_path / "missing.ply")
    write_ply_f4(missing, [names[i] for i in keep], block[:, keep])
    with pytest.raises(ValueError, match="rot_2"):
        si.load_gaussian_ply(missing, 1)
    vertex = np.zeros(3, dtype=[(n, "f8" if n == "opacity" else "f4") for n in names])
    double = str(tmp_path / "double.ply")
    write_ply(double, vertex)
    with pytest.raises(ValueError, match="not float"):
        si.load_gaussian_ply(double, 1)
    ascii_ = str(tmp_path / "ascii.ply")
    write_ply(ascii_, np.zeros(3, dtype=[(n, "f4") for n in names]), text=True)
    with pytest.raises(ValueError, match="ascii"):
        si.load_gaussian_ply(ascii_, 1)
    big = str(tmp_path / "big.ply")
    with open(good, "rb") as f, open(big, "wb") as g:
        g.write(f.read().replace(b"binary_little_endian", b"binary_big_endian"))
    with pytest.raises(ValueError, match="binary_big_endian"):
        si.load_gaussian_ply(big, 1)
    short = str(tmp_path / "short.ply")
    with open(good, "rb") as f, open(short, "wb") as g:
        g.write(f.read()[:-8])
    with pytest.raises(ValueError, match="truncated"):
        si.load_gaussian_ply(short, 1)
    with pytest.raises(ValueError, match="point_cloud"):
        si.load_checkpoint(str(tmp_path), 1)


def test_load_checkpoint_picks_the_largest_iteration(tmp_path):
    names = attribute_names(1)
    for it, n in ((7000, 2), (30000, 5), (900, 3)):
        d = tmp_path / "point_cloud" / f"iteration_{it}"
        os.makedirs(d)
        write_ply_f4(str(d / "point_cloud.ply"), names, np.full((n, len(names)), it, np.float32))
    assert len(si.load_checkpoint(str(tmp_path), 0)) == 5
    assert len(si.load_checkpoint(str(tmp_path), 0, iteration=900)) == 3


@pytest.mark.parametrize("case", ir.CASES)
def test_rotation_matrices_are_bit_equal_to_the_reference(case):
    cfg = ir.golden_config(case)
    mats = si.generate_rotation_matrices(cfg["rotation_degree"], cfg["rotation_axis"])
    want = ir.golden()[f"{case}/f32/rotation_matrices"]
    assert len(mats) == len(want)
    for m, w in zip(mats, want):
        assert m.dtype == torch.float32 and np.array_equal(m.numpy(), w)
    with pytest.raises(ValueError):
        si.generate_rotation_matrices([1.0], [3])


def test_load_params_from_gs_keys():
    """the switch and the keys, on a stand-in with the accessors (no device needed)"""
    import types
    pc = types.SimpleNamespace(get_xyz=torch.ones(2, 3), get_opacity=torch.ones(2, 1), get_features=torch.ones(2, 4, 3),
                               get_scaling=torch.ones(2, 3), get_rotation=torch.ones(2, 4), get_covariance=lambda m=1: torch.full((2, 6), float(m)))
    p = si.load_params_from_gs(pc, types.SimpleNamespace(compute_cov3D_python=True), scaling_modifier=2.0)
    assert set(p) == {"pos", "screen_points", "shs", "colors_precomp", "opacity", "scales", "rotations", "cov3D_precomp"}
    assert p["scales"] is None and p["rotations"] is None and float(p["cov3D_precomp"][0, 0]) == 2.0 and not p["screen_points"].any()
    p = si.load_params_from_gs(pc, types.SimpleNamespace(compute_cov3D_python=False), override_color=torch.zeros(2, 3))
    assert p["cov3D_precomp"] is None and p["scales"] is not None and p["shs"] is None and p["colors_precomp"] is not None
