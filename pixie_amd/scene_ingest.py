"""Scene ingest: a trained 3DGS checkpoint and a scene config to the particles the solver loads and the static tail the rasteriser
draws -- everything gs_simulation.py does in front of fill_particles (:363, :403-440).

Drop-ins for what that span calls:
  * `load_checkpoint(model_path, sh_degree=3, iteration=-1)` (gs_simulation.py:215-227) and `load_gaussian_ply(path, sh_degree=3)`
    (GaussianModel.load_ply): the PLY header is parsed here and the body is taken with ONE np.fromfile, as the (N, A) float32 block
    it is; columns are found by name, so permuted or extra columns are fine.  The result, a `GaussianCheckpoint`, has the accessors
    the frame loop reads from GaussianModel.
  * `load_params_from_gs(pc, pipe, scaling_modifier=1.0, override_color=None)` (utils/render_utils.py:59-110).
  * `generate_rotation_matrices(degrees, axes)` (utils/transformation_utils.py:23-51).
And for the statements :405-438 -- opacity filter, rotations, sim_area crop, transform2origin, shift2center111, covariance rotation and
scaling -- `ingest_scene`: the uploaded block goes through pixie_scene_ingest (csrc/scene_ingest.hip: classify + bound, scan, one
synchronise, emit) and comes back as an `IngestedScene`, selected Gaussians first and the unselected ones behind them in the same
buffers, so that the `torch.cat`s of :602-606 are views.

Differences from the reference, on purpose:
  * a selection of zero extent (one selected Gaussian included) is refused; the reference divides by zero there;
  * Gaussians whose opacity or rotated coordinate lies within float32 rounding of a threshold may classify differently from a torch
    run (the device's expf and the unfused rotation are not torch's kernels).
There is no CPU compute path.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib

_GEOMETRY = ["x", "y", "z", "opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
MAX_ROTATIONS = 8


def _read_header(path: str):
    """(format, [(element, count, [(type, name)])], offset of the body) of a PLY file"""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        fmt, elements = None, []
        while True:
            line = f.readline()
            if not line:
                raise ValueError(f"{path}: unterminated PLY header")
            tok = line.decode("ascii", "replace").split()
            if not tok or tok[0] in ("comment", "obj_info"):
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                if not elements:
                    raise ValueError(f"{path}: property before any element")
                elements[-1][2].append((" ".join(tok[1:-1]), tok[-1]))
            elif tok[0] == "end_header":
                return fmt, elements, f.tell()


def _sh_columns(names: List[str], sh_degree: int, path: str) -> List[str]:
    rest = sorted((n for n in names if n.startswith("f_rest_")), key=lambda n: int(n.split("_")[-1]))
    want = 3 * (sh_degree + 1) ** 2 - 3
    if len(rest) != want:
        raise ValueError(f"{path}: {len(rest)} f_rest_* properties, SH degree {sh_degree} needs {want}")
    return ["f_dc_0", "f_dc_1", "f_dc_2"] + rest


class GaussianCheckpoint:
    """What the frame loop reads from GaussianModel after load_ply, over the PLY body kept as one (N, A) float32 block.  Device
    tensors are made lazily: the block is uploaded once per device, and every accessor is a few torch expressions on it (these are
    conveniences for `load_params_from_gs`, `convert_SH` and `initialize_resterize`-style callers; `ingest_scene` reads the block)."""

    def __init__(self, block: np.ndarray, names: List[str], sh_degree: int, path: str = "<memory>"):
        if not 0 <= int(sh_degree) <= 3:
            raise ValueError(f"sh_degree {sh_degree} outside 0..3")
        self.block = np.ascontiguousarray(block, dtype=np.float32)
        self.names = list(names)
        self.path = path
        if self.block.ndim != 2 or self.block.shape[1] != len(self.names):
            raise ValueError(f"{path}: block of shape {self.block.shape} for {len(self.names)} properties")
        self.max_sh_degree = int(sh_degree)
        self.active_sh_degree = int(sh_degree)
        index = {n: i for i, n in reversed(list(enumerate(self.names)))}
        wanted = _GEOMETRY + _sh_columns(self.names, self.max_sh_degree, path)
        missing = [n for n in wanted if n not in index]
        if missing:
            raise ValueError(f"{path}: missing PLY properties {missing}")
        self.columns = np.array([index[n] for n in wanted], dtype=np.int32)   # the table pixie_scene_ingest takes
        self._device_blocks = {}

    def __len__(self):
        return int(self.block.shape[0])

    @property
    def n_sh_coeffs(self) -> int:
        return (self.max_sh_degree + 1) ** 2

    def device_block(self, device=None) -> torch.Tensor:
        device = _device(device)
        if device not in self._device_blocks:
            self._device_blocks[device] = torch.from_numpy(self.block).to(device)
        return self._device_blocks[device]

    def _cols(self, lo, hi):
        idx = torch.as_tensor(self.columns[lo:hi].astype(np.int64))
        blk = self.device_block()
        return blk[:, idx.to(blk.device)]

    @property
    def get_xyz(self):
        return self._cols(0, 3)

    @property
    def get_opacity(self):
        return torch.sigmoid(self._cols(3, 4))

    @property
    def get_scaling(self):
        return torch.exp(self._cols(4, 7))

    @property
    def get_rotation(self):
        return torch.nn.functional.normalize(self._cols(7, 11))

    @property
    def get_features(self):
        k = self.n_sh_coeffs
        dc = self._cols(11, 14).unsqueeze(1)                                          # (N, 1, 3)
        rest = self._cols(14, 11 + 3 * k).reshape(len(self), 3, k - 1).transpose(1, 2)    # (N, K - 1, 3)
        return torch.cat((dc, rest), dim=1).contiguous()

    def get_covariance(self, scaling_modifier=1):
        """build_covariance_from_scaling_rotation: (R S)(R S)^T of scaling_modifier * exp(scale) and the normalised quaternion, as
        its 6 upper entries"""
        s = scaling_modifier * self.get_scaling
        q = self._cols(7, 11)
        q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
        L = R * s[:, None, :]
        cov = L @ L.transpose(1, 2)
        return torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], dim=1)


def load_gaussian_ply(path: str, sh_degree: int = 3) -> GaussianCheckpoint:
    """GaussianModel(sh_degree).load_ply(path): the first element of a binary little-endian PLY whose properties are all float32."""
    fmt, elements, offset = _read_header(path)
    if fmt != "binary_little_endian":
        raise ValueError(f"{path}: PLY format {fmt!r}; a checkpoint is binary_little_endian")
    if not elements:
        raise ValueError(f"{path}: no element")
    _, count, props = elements[0]
    bad = [(t, n) for t, n in props if t not in ("float", "float32")]
    if bad:
        raise ValueError(f"{path}: properties that are not float: {bad}")
    names = [n for _, n in props]
    # the checks that need only the header come before the body is read
    ck_names = _GEOMETRY + _sh_columns(names, int(sh_degree), path)
    missing = [n for n in ck_names if n not in names]
    if missing:
        raise ValueError(f"{path}: missing PLY properties {missing}")
    block = np.fromfile(path, dtype="<f4", count=count * len(names), offset=offset)
    if block.size != count * len(names):
        raise ValueError(f"{path}: truncated body: {block.size} of {count * len(names)} floats")
    return GaussianCheckpoint(block.reshape(count, len(names)), names, int(sh_degree), path)


def _checkpoint_path(model_path: str, iteration: int = -1) -> str:
    checkpt_dir = os.path.join(model_path, "point_cloud")
    if not os.path.isdir(checkpt_dir):
        raise ValueError(f"{model_path}: no point_cloud directory")
    if iteration == -1:
        saved = [int(f.split("_")[-1]) for f in os.listdir(checkpt_dir) if f.split("_")[-1].isdigit()]
        if not saved:
            raise ValueError(f"{checkpt_dir}: no iteration_<n> directory")
        iteration = max(saved)
    path = os.path.join(checkpt_dir, f"iteration_{iteration}", "point_cloud.ply")
    if not os.path.isfile(path):
        raise ValueError(f"{path}: no such checkpoint")
    return path


def load_checkpoint(model_path: str, sh_degree: int = 3, iteration: int = -1) -> GaussianCheckpoint:
    """gs_simulation.py:215-227: <model_path>/point_cloud/iteration_<iteration, the largest if -1>/point_cloud.ply"""
    return load_gaussian_ply(_checkpoint_path(model_path, iteration), sh_degree)


def load_params_from_gs(pc, pipe, scaling_modifier=1.0, override_color=None):
    """utils/render_utils.py:59-110, inference only: screen_points is zeros and carries no gradient"""
    means3D = pc.get_xyz
    scales = rotations = cov3D_precomp = None
    if pipe.compute_cov3D_python:
        cov3D_precomp = pc.get_covariance(scaling_modifier)
    else:
        scales, rotations = pc.get_scaling, pc.get_rotation
    shs = colors_precomp = None
    if override_color is None:
        shs = pc.get_features
    else:
        colors_precomp = override_color
    return {"pos": means3D, "screen_points": torch.zeros_like(means3D), "shs": shs, "colors_precomp": colors_precomp,
            "opacity": pc.get_opacity, "scales": scales, "rotations": rotations, "cov3D_precomp": cov3D_precomp}


def generate_rotation_matrices(degrees, axes, device=None) -> List[torch.Tensor]:
    """utils/transformation_utils.py:23-51 with its arithmetic -- float32, pi = 3.1415926, torch's cos / sin on the host, so the
    matrices do not depend on the device -- as (3, 3) float32 tensors on `device` (the host if None)."""
    degrees = torch.as_tensor(degrees).detach().cpu()
    if not degrees.is_floating_point():
        degrees = degrees.to(torch.float32)
    degrees = degrees.reshape(-1)
    assert len(degrees) == len(axes)
    out = []
    for degree, axis in zip(degrees, axes):
        c = torch.cos(degree / 180.0 * 3.1415926)
        s = torch.sin(degree / 180.0 * 3.1415926)
        if axis == 0:
            m = torch.tensor([[1, 0, 0], [0, c, -s], [0, s, c]])
        elif axis == 1:
            m = torch.tensor([[c, 0, s], [0, 1, 0], [-s, 0, c]])
        elif axis == 2:
            m = torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1]])
        else:
            raise ValueError("Invalid axis selection")
        out.append(m.to(torch.float32) if device is None else m.to(torch.float32).to(device))
    return out


@dataclass
class IngestedScene:
    """The state gs_simulation.py holds at :440.  `pos`, `cov`, `opacity`, `shs` are the selected Gaussians in the solver frame --
    what fill_particles and load_initial_data_from_torch take; `unselected` the static tail in the scene frame, or None.  All are
    views of four buffers in which the unselected rows follow the selected ones, so `opacity_all` / `shs_all` (and
    `torch.cat([pos_render, unselected[0]])`'s static half) need no copy in the frame loop."""
    pos: torch.Tensor
    cov: torch.Tensor
    opacity: torch.Tensor
    shs: torch.Tensor
    unselected: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]]
    opacity_all: torch.Tensor
    shs_all: torch.Tensor
    gs_num: int
    scale_origin: float
    original_mean_pos: torch.Tensor
    rotation_matrices: List[torch.Tensor]
    z_shift_value: float
    n_loaded: int
    n_dropped: int


def _device(device) -> torch.device:
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.PixieHipError("scene_ingest: no HIP device is visible (there is no CPU path)")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("scene_ingest: device must be a HIP device (there is no CPU path)")
    return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())


def _sh_degree_of(path: str) -> int:
    _, elements, _ = _read_header(path)
    n_rest = sum(1 for _, n in (elements[0][2] if elements else []) if n.startswith("f_rest_"))
    for degree in range(4):
        if 3 * (degree + 1) ** 2 - 3 == n_rest:
            return degree
    raise ValueError(f"{path}: {n_rest} f_rest_* properties fit no SH degree 0..3")


_REFUSALS = {
    _lib.INGEST_NO_SELECTION: "no Gaussian passes the opacity filter inside sim_area, so there is nothing to simulate",
    _lib.INGEST_ZERO_EXTENT: "the selected Gaussians have zero extent (a single one, or all at one point), so transform2origin's scale "
                             "1 / max(max - min) is not finite",
    _lib.INGEST_TOO_MANY_ROTATIONS: f"more than {MAX_ROTATIONS} rotations",
    _lib.INGEST_TOO_MANY_ROWS: "more than 2^31 - 2 Gaussians",
}


def ingest_scene(checkpoint_or_path, preprocessing_params, device=None) -> IngestedScene:
    """gs_simulation.py:405-438 on the device.  `checkpoint_or_path`: a GaussianCheckpoint, a model directory (load_checkpoint's
    rule) or a PLY file (its SH degree follows from its f_rest_* count).  Keys read from `preprocessing_params`: opacity_threshold,
    rotation_degree, rotation_axis, sim_area (None or absent: everything that passes the opacity filter is selected) and
    z_shift_value (default 0).  One stream synchronise; the outputs are ready on the current stream."""
    if isinstance(checkpoint_or_path, GaussianCheckpoint):
        ck = checkpoint_or_path
    else:
        path = os.fspath(checkpoint_or_path)
        if os.path.isdir(path):
            path = _checkpoint_path(path)
        ck = load_gaussian_ply(path, _sh_degree_of(path))
    device = _device(device)
    p = preprocessing_params
    degrees, axes = list(p.get("rotation_degree", [])), list(p.get("rotation_axis", []))
    if len(degrees) != len(axes):
        raise ValueError(f"rotation_degree has {len(degrees)} entries, rotation_axis {len(axes)}")
    rots = generate_rotation_matrices(torch.tensor(degrees, dtype=torch.float32) if degrees else torch.zeros(0), axes)
    area = p.get("sim_area")
    if area is not None and len(area) != 6:
        raise ValueError(f"sim_area must be (x0, x1, y0, y1, z0, z1); got {area}")
    z_shift = float(p.get("z_shift_value", 0.0))

    n, k = len(ck), ck.n_sh_coeffs
    block = ck.device_block(device)
    pos = torch.empty((n, 3), dtype=torch.float32, device=device)
    cov = torch.empty((n, 6), dtype=torch.float32, device=device)
    opacity = torch.empty((n, 1), dtype=torch.float32, device=device)
    shs = torch.empty((n, k, 3), dtype=torch.float32, device=device)

    lib = _lib.load()
    d = _lib.IngestDesc()
    d.n, d.n_attr, d.sh_degree = n, int(ck.block.shape[1]), ck.max_sh_degree
    d.n_rotations, d.has_sim_area = len(rots), int(area is not None)
    flat = np.concatenate([r.numpy().reshape(-1) for r in rots[:MAX_ROTATIONS]]) if rots else np.zeros(0, np.float32)
    for i, v in enumerate(flat):
        d.rotations[i] = float(v)
    for i, v in enumerate(area if area is not None else [0.0] * 6):
        d.sim_area[i] = float(v)
    d.opacity_threshold, d.z_shift = float(p["opacity_threshold"]), z_shift
    d.d_block = block.data_ptr()
    d.columns = ck.columns.ctypes.data_as(C.POINTER(C.c_int32))
    d.d_pos, d.d_cov, d.d_opacity, d.d_shs = pos.data_ptr(), cov.data_ptr(), opacity.data_ptr(), shs.data_ptr()
    counts, scale, mean = (C.c_int64 * 3)(), (C.c_float * 1)(), (C.c_float * 3)()
    with torch.cuda.device(device):
        ws_bytes = 0
        if len(rots) <= MAX_ROTATIONS and 0 < n <= 2 ** 31 - 2:
            ws_bytes = int(lib.pixie_scene_ingest_workspace_bytes(n))
            if ws_bytes < 0:
                _lib.check(1, "pixie_scene_ingest_workspace_bytes", lib=lib)
        workspace = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
        d.d_workspace, d.workspace_bytes = workspace.data_ptr(), ws_bytes
        rc = lib.pixie_scene_ingest(C.byref(d), counts, scale, mean, _lib.current_stream_ptr())
    if rc in _REFUSALS:
        raise ValueError(f"ingest_scene({ck.path}): {_REFUSALS[rc]}")
    _lib.check(rc, "pixie_scene_ingest", lib=lib)

    n_sel, n_unsel, n_drop = int(counts[0]), int(counts[1]), int(counts[2])
    end = n_sel + n_unsel
    sel = (pos[:n_sel], cov[:n_sel], opacity[:n_sel], shs[:n_sel])
    if n_unsel:
        unselected = (pos[n_sel:end], cov[n_sel:end], opacity[n_sel:end], shs[n_sel:end])
        opacity_all, shs_all = opacity[:end], shs[:end]
    else:
        unselected, opacity_all, shs_all = None, sel[2], sel[3]
    return IngestedScene(pos=sel[0], cov=sel[1], opacity=sel[2], shs=sel[3], unselected=unselected, opacity_all=opacity_all,
                         shs_all=shs_all, gs_num=n_sel, scale_origin=float(scale[0]),
                         original_mean_pos=torch.tensor([mean[0], mean[1], mean[2]], dtype=torch.float32).to(device),
                         rotation_matrices=[r.to(device) for r in rots], z_shift_value=z_shift, n_loaded=n, n_dropped=n_drop)
