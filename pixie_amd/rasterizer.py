"""Forward 3D Gaussian splatting rasteriser: the per-frame render of gs_simulation.py's frame loop (:590, :610-619, :630-631).

Drop-ins for what that loop imports:
  * `GaussianRasterizationSettings`, `GaussianRasterizer` (diff_gaussian_rasterization/__init__.py:157-220): same fields, same call
    signature, same two argument errors, (color (3, H, W), radii (N,)) back.  Forward only: nothing differentiates through a render
    in the simulation, and the outputs carry no graph.
  * `convert_SH` (utils/render_utils.py:113-130): one launch (pixie_sh_to_rgb) instead of the torch expression.
And for `SceneBatch.run_frames` results: `render_frames`; for the frame files: `save_frame_png`.

Differences from the reference, on purpose:
  * Gaussians with equal (tile, depth) are blended in index order (a stable sort), so an image is reproducible bit for bit;
  * `means2D` is ignored (upstream it only carries a gradient);
  * `prefiltered` and `debug` are accepted and unused.
There is no CPU compute path: a host tensor is refused.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _lib


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _device_f32(t, what, shape_tail, n=None):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise ValueError(f"{what} must be a tensor on a HIP device (there is no CPU path)")
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    t = t.reshape((-1,) + tuple(shape_tail)) if n is None else t.reshape((n,) + tuple(shape_tail))
    return t.contiguous()


def _host_floats(t, count, what):
    v = torch.as_tensor(t).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    if v.numel() != count:
        raise ValueError(f"{what} must hold {count} values, got {v.numel()}")
    return [float(x) for x in v]


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def sh_to_rgb(shs, degree, position, campos, rotation=None):
    """max(SH_degree(shs; normalise(position - campos)) + 0.5, 0): shs (N, K, 3), position (N, 3) on a HIP device, K >= (degree+1)^2;
    `rotation` (n <= N, 3, 3) rotates the first n directions.  Returns (N, 3) float32, asynchronously on the current stream."""
    pos = _device_f32(position, "sh_to_rgb: position", (3,))
    n = pos.shape[0]
    shs = _device_f32(shs, "sh_to_rgb: shs", tuple(shs.shape[1:]) if torch.is_tensor(shs) else (), n)
    if shs.dim() != 3 or shs.shape[2] != 3:
        raise ValueError(f"sh_to_rgb: shs must be (N, K, 3), got {tuple(shs.shape)}")
    rot = None if rotation is None else _device_f32(rotation, "sh_to_rgb: rotation", (3, 3))
    out = torch.empty((n, 3), dtype=torch.float32, device=pos.device)
    lib = _lib.load()
    cam = (C.c_float * 3)(*_host_floats(campos, 3, "sh_to_rgb: campos"))
    with torch.cuda.device(pos.device):
        rc = lib.pixie_sh_to_rgb(_ptr(shs), n, int(shs.shape[1]), int(degree), _ptr(pos), cam, _ptr(rot), 0 if rot is None else int(rot.shape[0]),
                                 _ptr(out), _lib.current_stream_ptr())
    _lib.check(rc, "pixie_sh_to_rgb", lib=lib)
    return out


def convert_SH(shs_view, viewpoint_camera, pc, position, rotation=None):
    """utils/render_utils.py:113-130.  shs_view: (N, (pc.max_sh_degree + 1)^2, 3); evaluated up to pc.active_sh_degree along
    position - viewpoint_camera.camera_center.  Uses nothing else of `viewpoint_camera` and `pc`."""
    k = (int(pc.max_sh_degree) + 1) ** 2
    if not torch.is_tensor(shs_view) or shs_view.dim() != 3 or shs_view.shape[1] != k or shs_view.shape[2] != 3:
        raise ValueError(f"convert_SH: shs_view must be (N, {k}, 3) for max_sh_degree {pc.max_sh_degree}, got "
                         f"{tuple(shs_view.shape) if torch.is_tensor(shs_view) else type(shs_view)}")
    return sh_to_rgb(shs_view, int(pc.active_sh_degree), position, viewpoint_camera.camera_center, rotation)


class GaussianRasterizer(torch.nn.Module):
    """`GaussianRasterizer(raster_settings)(means3D, means2D, opacities, ...)` -> (color (3, H, W), radii (N,) int32).
    The workspace is kept between calls and grows when a render needs more instances (Gaussian-tile pairs) than it holds.
    After a call, `last_instances` is that render's instance count; `forward(..., aux=True)` also returns (final_T, n_contrib)."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings
        self._workspace = None
        self._capacity = 0             # instances the workspace was sized for
        self._key = None
        self._host = None              # (settings object, viewmatrix, projmatrix, bg as ctypes arrays): read back once per settings
        self.last_instances = 0

    def _ensure_workspace(self, lib, n, device, instances):
        s = self.raster_settings
        key = (n, int(s.image_width), int(s.image_height), device)
        if self._workspace is not None and self._key == key and self._capacity >= instances:
            return
        need = lib.pixie_raster_workspace_bytes(n, key[1], key[2], int(instances))
        if need < 0:
            _lib.check(1, "pixie_raster_workspace_bytes", lib=lib)
        self._workspace = torch.empty((max(int(need), 16),), dtype=torch.uint8, device=device)
        self._capacity, self._key = int(instances), key

    def _host_settings(self):
        s = self.raster_settings
        if self._host is None or self._host[0] is not s:
            self._host = (s, (C.c_float * 16)(*_host_floats(s.viewmatrix, 16, "GaussianRasterizer: viewmatrix")),
                          (C.c_float * 16)(*_host_floats(s.projmatrix, 16, "GaussianRasterizer: projmatrix")),
                          (C.c_float * 3)(*_host_floats(s.bg, 3, "GaussianRasterizer: bg")),
                          torch.as_tensor(s.campos).detach().to(device="cpu", dtype=torch.float32).reshape(-1))
        return self._host

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None,
                out=None, aux=False):
        s = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        means = _device_f32(means3D, "GaussianRasterizer: means3D", (3,))
        n, device = means.shape[0], means.device
        if shs is not None:
            colors = sh_to_rgb(shs, int(s.sh_degree), means, self._host_settings()[4])
        else:
            colors = _device_f32(colors_precomp, "GaussianRasterizer: colors_precomp", (3,), n)
        opac = _device_f32(opacities, "GaussianRasterizer: opacities", (), n)
        cov = sc = rot = None
        if cov3D_precomp is not None:
            cov = _device_f32(cov3D_precomp, "GaussianRasterizer: cov3D_precomp", (6,), n)
        else:
            sc = _device_f32(scales, "GaussianRasterizer: scales", (3,), n)
            rot = _device_f32(rotations, "GaussianRasterizer: rotations", (4,), n)
        H, W = int(s.image_height), int(s.image_width)
        if out is None:
            out = torch.empty((3, H, W), dtype=torch.float32, device=device)
        elif out.shape != (3, H, W) or out.dtype != torch.float32 or out.device != device or not out.is_contiguous():
            raise ValueError(f"GaussianRasterizer: out must be a contiguous float32 (3, {H}, {W}) tensor on {device}")
        radii = torch.empty((n,), dtype=torch.int32, device=device)
        final_T = torch.empty((H, W), dtype=torch.float32, device=device) if aux else None
        n_contrib = torch.empty((H, W), dtype=torch.int32, device=device) if aux else None

        lib = _lib.load()
        d = _lib.RasterDesc()
        d.n, d.width, d.height = n, W, H
        d.tanfovx, d.tanfovy, d.scale_modifier = float(s.tanfovx), float(s.tanfovy), float(s.scale_modifier)
        _, d.viewmatrix, d.projmatrix, d.bg, _ = self._host_settings()
        for name, t in (("d_means", means), ("d_cov3d", cov), ("d_scales", sc), ("d_rotations", rot), ("d_colors", colors),
                        ("d_opacity", opac), ("d_radii", radii), ("d_final_T", final_T), ("d_n_contrib", n_contrib)):
            setattr(d, name, t.data_ptr() if t is not None and t.numel() else None)
        d.d_out_color = out.data_ptr()
        count = C.c_int64(0)
        with torch.cuda.device(device):
            same = self._key == (n, W, H, device)
            self._ensure_workspace(lib, n, device, self._capacity if same else 4 * n)      # a first guess: four tiles per Gaussian
            for attempt in (0, 1):
                d.d_workspace, d.workspace_bytes = self._workspace.data_ptr(), self._workspace.numel()
                rc = lib.pixie_raster_forward(C.byref(d), C.byref(count), _lib.current_stream_ptr())
                if rc == 0 or attempt == 1 or count.value <= 0:
                    break
                # Too small?  Decided in bytes, not instances: the library's sort storage need not grow monotonically with the count.
                grown = count.value + count.value // 2
                need = max(lib.pixie_raster_workspace_bytes(n, W, H, count.value), lib.pixie_raster_workspace_bytes(n, W, H, grown))
                if need <= self._workspace.numel():
                    break                                  # the call failed for another reason: report it
                self._workspace = torch.empty((int(need),), dtype=torch.uint8, device=device)      # grow to 1.5 x and retry once
                self._capacity = grown
        _lib.check(rc, "pixie_raster_forward", lib=lib)
        self.last_instances = int(count.value)
        return (out, radii, final_T, n_contrib) if aux else (out, radii)


def render_frames(frames, settings_per_frame, opacity, shs=None, colors_precomp=None, unselected=None, rasterizer=None):
    """Renders what `SceneBatch.run_frames` returns for a scene -- (pos (F, N, 3), cov (F, N, 6), ...) -- into (F, 3, H, W) on the
    device; frame f equals `GaussianRasterizer(settings_f)(pos[f], None, opacity, shs or colors_precomp, cov3D_precomp=cov[f])` bit
    for bit.  `settings_per_frame`: one GaussianRasterizationSettings, or one per frame (a moving camera) with one image size.
    Exactly one of `shs` (N', K, 3; evaluated per frame at sh_degree from campos) and `colors_precomp` (N', 3).
    `unselected`: (pos (M, 3), cov (M, 6)) of Gaussians that do not simulate, appended to every frame (gs_simulation.py:602-606);
    `opacity` and the colours then cover N' = N + M Gaussians."""
    pos, cov = frames[0], frames[1]
    if cov is None:
        raise ValueError("render_frames: the frames carry no covariance (FrameSchedule.with_cov)")
    if (shs is None) == (colors_precomp is None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    n_frames = int(pos.shape[0])
    per_frame = None if isinstance(settings_per_frame, GaussianRasterizationSettings) else list(settings_per_frame)
    if per_frame is not None and len(per_frame) != n_frames:
        raise ValueError(f"render_frames: {len(per_frame)} settings for {n_frames} frames")
    first = per_frame[0] if per_frame else settings_per_frame
    H, W = int(first.image_height), int(first.image_width)
    if not torch.is_tensor(pos) or pos.device.type != "cuda":
        raise ValueError("render_frames: frames must be tensors on a HIP device (there is no CPU path)")
    out = torch.empty((n_frames, 3, H, W), dtype=torch.float32, device=pos.device)
    r = rasterizer if rasterizer is not None else GaussianRasterizer(first)
    for f in range(n_frames):
        s = per_frame[f] if per_frame else first
        if (int(s.image_height), int(s.image_width)) != (H, W):
            raise ValueError("render_frames: every frame must have the same image size")
        r.raster_settings = s
        p, c = pos[f], cov[f]
        if unselected is not None:
            p = torch.cat([p, unselected[0].to(p.device, torch.float32)], dim=0)
            c = torch.cat([c, unselected[1].to(c.device, torch.float32)], dim=0)
        r(p, None, opacity, shs=shs, colors_precomp=colors_precomp, cov3D_precomp=c, out=out[f])
    return out


def save_frame_png(path, image):
    """Writes a (3, H, W) RGB image with values in [0, 1] as an 8-bit PNG: round(clip(255 x, 0, 255)), the file the reference's
    cvtColor + imwrite pair produces for frames/%05d.png.  Returns the path."""
    if not torch.is_tensor(image) or image.dim() != 3 or image.shape[0] != 3:
        raise ValueError("save_frame_png: image must be a (3, H, W) tensor")
    try:
        from PIL import Image
    except ImportError as exc:
        raise RuntimeError("save_frame_png needs Pillow (PIL), which is not installed") from exc
    a = (image.detach().float() * 255.0).clamp(0.0, 255.0).round().to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy()
    Image.fromarray(a).save(path, format="PNG")
    return path
