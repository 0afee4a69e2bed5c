"""CPU checks of the per-frame splat PLY (pixie_amd/splat_export.py): the vertex block and the file export_gaussians_to_ply's
writer produces equal, bit for bit, what the reference's GaussianModel.save_ply assembles (recorded in
tests/golden/splat_export.npz at SH degrees 0 and 3), given the same scales and quaternions."""
import numpy as np
import pytest
import torch

from pixie_amd import ply_io, splat_export
from tests import _splat_checks as sc


@pytest.mark.parametrize("deg", [0, 3])
def test_vertex_block_and_file_match_save_ply(deg, tmp_path):
    g = sc.golden()
    names = [str(n) for n in g[f"ply{deg}/names"]]
    ref = g[f"ply{deg}/elements"]
    assert list(ref.dtype.names) == names and all(ref.dtype[n] == np.dtype("f4") for n in names)
    assert len(names) == 17 + 3 * ((deg + 1) ** 2 - 1)
    t = lambda k: torch.from_numpy(g[f"ply{deg}/{k}"])
    block, got_names = splat_export.vertex_block(t("xyz"), t("scale"), t("rot"), t("opacity"), t("shs"))
    assert got_names == names
    assert block.dtype == torch.float32 and tuple(block.shape) == (len(ref), len(names))
    ref_block = ref.view(np.float32).reshape(len(ref), len(names))      # all-f4 structured rows are the same bytes
    assert np.array_equal(block.numpy().view(np.uint32), ref_block.view(np.uint32))

    path = splat_export.write_vertex_block(str(tmp_path / "frame_00003.ply"), block, got_names)
    raw = open(path, "rb").read()
    header = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(ref)
              + "".join(f"property float {n}\n" for n in names) + "end_header\n").encode("ascii")
    assert raw[:len(header)] == header
    assert raw[len(header):] == ref.astype(np.dtype([(n, "<f4") for n in names])).tobytes()
    # the same bytes as the general writer (plyfile's layout) of the recorded array
    ply_io.write_ply(str(tmp_path / "ref.ply"), ref)
    assert open(tmp_path / "ref.ply", "rb").read() == raw
    back, _ = ply_io.read_ply(path)
    assert back.dtype.names == ref.dtype.names
    assert np.array_equal(back.view(np.uint32), ref.view(np.uint32))


def test_write_splat_frames_names_and_order(tmp_path):
    """run_frames layout (n_frames, gs_num, .) -> one frame_{f:05d}.ply per frame, rows as the single-frame writer's"""
    g = sc.golden()
    t = lambda k: torch.from_numpy(g[f"ply3/{k}"])
    n = t("xyz").shape[0]
    pos = torch.stack([t("xyz"), t("xyz") + 1])
    frames = (pos, torch.zeros((2, n, 6)), torch.stack([t("scale")] * 2), torch.stack([t("rot")] * 2))
    paths = splat_export.write_splat_frames(str(tmp_path / "ply_files"), frames, t("opacity"), t("shs"), 3, first_frame=7)
    assert [p.rsplit("/", 1)[1] for p in paths] == ["frame_00007.ply", "frame_00008.ply"]
    for f, p in enumerate(paths):
        v, _ = ply_io.read_ply(p)
        assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), pos[f].numpy())
        assert np.array_equal(v["rot_2"], g["ply3/rot"][:, 2]) and np.array_equal(v["f_rest_44"], g["ply3/elements"]["f_rest_44"])


def test_no_cpu_compute_path():
    with pytest.raises(ValueError, match="HIP device"):
        splat_export.cov3D_to_log_scales_and_quats(torch.zeros((4, 6)))
