"""Per-frame 3D Gaussian splat export: the PLY files gs_simulation.py writes every frame with `--save_ply` (its default config).

Drop-ins for the two functions gs_simulation.py defines for it:
  * `cov3D_to_log_scales_and_quats(cov3D)` (gs_simulation.py:253-288): eigen-decomposition of every covariance into log-scales
    and a wxyz quaternion -- on the device (pixie_splat_from_cov, one launch); the reference runs torch.linalg.eigh and then
    scipy on the host.
  * `export_gaussians_to_ply(...)` (gs_simulation.py:290-322): the frame's positions, covariances and splats from ONE launch
    (MPM_Simulator_WARP.export_frame_splats), the vertex block of GaussianModel.save_ply
    (gaussian-splatting/scene/gaussian_model.py:177-208) assembled on the device, one device-to-host copy, one file write.
And for `SceneBatch.run_frames` results with `FrameSchedule(with_splats=True)`: `write_splat_frames`.

Differences from the reference, on purpose:
  * quaternions are float32 (the reference's come from scipy as float64; the PLY stores float32 either way);
  * eigenvector signs are fixed (include/pixie_hip.h, pixie_splat_from_cov) instead of whatever LAPACK returns, so the
    quaternion of a Gaussian is reproducible; any sign choice describes the same Gaussian.
There is no CPU compute path: a host tensor is refused.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from .ply_io import write_ply_f4


def cov3D_to_log_scales_and_quats(cov3D: torch.Tensor):
    """cov3D: (N, 6) float32 covariances (s11, s12, s13, s22, s23, s33) on a HIP device.  Returns (log_scales (N, 3) descending,
    quats (N, 4) wxyz, unit, w >= 0), both float32 on cov3D's device, asynchronously on the current stream."""
    if not torch.is_tensor(cov3D) or cov3D.device.type != "cuda":
        raise ValueError("cov3D_to_log_scales_and_quats: cov3D must be a tensor on a HIP device (there is no CPU path)")
    if cov3D.dtype != torch.float32 or cov3D.dim() != 2 or cov3D.shape[1] != 6:
        raise ValueError(f"cov3D_to_log_scales_and_quats: expected a float32 (N, 6) tensor, got {tuple(cov3D.shape)} {cov3D.dtype}")
    cov = cov3D.contiguous()
    n = cov.shape[0]
    ls = torch.empty((n, 3), dtype=torch.float32, device=cov.device)
    quat = torch.empty((n, 4), dtype=torch.float32, device=cov.device)
    if n == 0:
        return ls, quat
    lib = _lib.load()
    with torch.cuda.device(cov.device):
        rc = lib.pixie_splat_from_cov(C.c_void_p(cov.data_ptr()), n, C.c_void_p(ls.data_ptr()), C.c_void_p(quat.data_ptr()),
                                      _lib.current_stream_ptr())
    _lib.check(rc, "pixie_splat_from_cov", lib=lib)
    return ls, quat


def attribute_names(n_sh_coeffs: int):
    """GaussianModel.construct_list_of_attributes for shs of shape (N, n_sh_coeffs, 3)"""
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)]
            + [f"f_rest_{i}" for i in range(3 * (n_sh_coeffs - 1))] + ["opacity"] + [f"scale_{i}" for i in range(3)]
            + [f"rot_{i}" for i in range(4)])


def _static_columns(opacity, shs, n, device):
    """(f_dc | f_rest | opacity) of save_ply: shs (n, K, 3) channel-major (transpose(1, 2).flatten(1)), opacity as given"""
    shs = torch.as_tensor(shs)[:n].to(device=device, dtype=torch.float32)
    if shs.dim() != 3 or shs.shape[2] != 3 or shs.shape[0] != n:
        raise ValueError(f"shs_render must be (N >= {n}, K, 3); got {tuple(shs.shape)}")
    op = torch.as_tensor(opacity)[:n].to(device=device, dtype=torch.float32).reshape(n, -1)
    if op.shape[1] != 1:
        raise ValueError(f"opacity_render must be (N >= {n}, 1); got {tuple(torch.as_tensor(opacity).shape)}")
    f_dc = shs[:, :1, :].transpose(1, 2).flatten(start_dim=1)
    f_rest = shs[:, 1:, :].transpose(1, 2).flatten(start_dim=1)
    return torch.cat([f_dc, f_rest, op], dim=1), int(shs.shape[1])


def vertex_block(pos, log_scales, quats, opacity, shs):
    """The (N, A) float32 rows save_ply writes -- x y z, nx ny nz (zero), f_dc_0..2, f_rest_*, opacity, scale_0..2, rot_0..3 --
    assembled on pos's device.  Returns (block, attribute names)."""
    n = pos.shape[0]
    static, k = _static_columns(opacity, shs, n, pos.device)
    block = torch.cat([pos.to(torch.float32), torch.zeros((n, 3), dtype=torch.float32, device=pos.device), static,
                       log_scales.to(torch.float32), quats.to(torch.float32)], dim=1)
    return block, attribute_names(k)


def write_vertex_block(path: str, block: torch.Tensor, names) -> str:
    """One device-to-host copy of the block and one file write (the layout plyfile writes for save_ply's element)."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    write_ply_f4(path, names, block.contiguous().cpu().numpy())
    return path


def export_gaussians_to_ply(ply_out_dir, mpm_solver, active_sh_degree, gs_num, scale_origin, rotation_matrices, opacity_render,
                            shs_render, frame, preprocessing_params, original_mean_pos, to_original_coord=True):
    """gs_simulation.py:290-322: writes ply_out_dir/frame_{frame:05d}.ply, save_ply's columns for the first gs_num Gaussians.
    Positions are the rasteriser's (original scene frame) with to_original_coord, otherwise the solver frame's
    export_particle_x_to_torch()[:gs_num]; the covariance -- hence scales and rotations -- is the original-frame one either way,
    as in the reference.  `opacity_render` is written as given (the reference's driver passes activated opacities).
    `active_sh_degree` is accepted for the signature; the column count follows shs_render, as save_ply's does.  Returns the path."""
    n = int(gs_num)
    pos, _cov, ls, quat = mpm_solver.export_frame_splats(n, scale_origin, original_mean_pos, rotation_matrices,
                                                         preprocessing_params["z_shift_value"])
    if not to_original_coord:
        pos = mpm_solver.export_particle_x_to_torch()[:n]
    block, names = vertex_block(pos, ls, quat, opacity_render, shs_render)
    return write_vertex_block(os.path.join(ply_out_dir, f"frame_{frame:05d}.ply"), block, names)


def write_splat_frames(ply_files_dir, frames, opacity_render, shs_render, active_sh_degree, first_frame=0):
    """Write a SceneBatch.run_frames result of a scene with with_splats -- (pos, cov, log_scales, quats), each (n_frames, gs_num, .)
    -- as the per-frame files of export_gaussians_to_ply: ply_files_dir/frame_{first_frame + f:05d}.ply.  Returns the paths."""
    pos, _cov, ls, quat = frames
    n_frames, n = int(pos.shape[0]), int(pos.shape[1])
    static, k = _static_columns(opacity_render, shs_render, n, pos.device)
    names = attribute_names(k)
    zeros = torch.zeros((n, 3), dtype=torch.float32, device=pos.device)
    paths = []
    for f in range(n_frames):
        block = torch.cat([pos[f], zeros, static, ls[f], quat[f]], dim=1)
        paths.append(write_vertex_block(os.path.join(ply_files_dir, f"frame_{first_frame + f:05d}.ply"), block, names))
    return paths
