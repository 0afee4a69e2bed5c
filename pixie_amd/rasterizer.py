"""3D Gaussian splatting rasteriser: the per-frame render of gs_simulation.py's frame loop (:590, :610-619, :630-631), and, through
torch autograd, the differentiable render that gaussian-splatting/train.py optimises through.

Drop-ins for what that loop imports:
  * `GaussianRasterizationSettings`, `GaussianRasterizer` (diff_gaussian_rasterization/__init__.py:157-220): same fields, same call
    signature, same two argument errors, (color (3, H, W), radii (N,)) back.  With grad mode on and an input that requires grad the
    colour carries a graph whose backward is one pixie_raster_backward call (HIP, include/pixie_hip.h section D'); otherwise, and
    always under torch.no_grad() or with `out=` given, the render is the forward-only one of the simulation loop, bit for bit.
  * `convert_SH` (utils/render_utils.py:113-130): one launch (pixie_sh_to_rgb) instead of the torch expression.
And for `SceneBatch.run_frames` results: `render_frames` (a call per frame) and `render_frame_batch` / `FrameBatchRasterizer` (the
whole sequence in one pixie_raster_forward_batch call: one stream synchronise however many frames, the same bits per image); for
the frame files: `save_frame_png`, `save_frame_pngs`.

What is differentiable: `GaussianRasterizer.forward` with respect to means3D, means2D, opacities, shs or colors_precomp, and scales and
rotations or cov3D_precomp.  What is not: `render_frames`, `render_frame_batch` and `FrameBatchRasterizer` stay forward-only; double
backward is not supported; the camera matrices, campos and bg get no gradient; final_T (aux=True) carries none.

Differences from the reference, on purpose:
  * Gaussians with equal (tile, depth) are blended in index order (a stable sort), so an image is reproducible bit for bit, and so
    are the gradients: the backward reduces in a fixed order and uses no floating-point atomics;
  * the gradient is the exact derivative of the forward with every discrete decision held fixed, which differs from upstream's
    backward.cu in three small places: no gradient through an active min(0.99, .), the Jacobian term under an active 1.3 tanfov
    clamp is differentiated as the forward computes it, and no 1e-7 is added to the determinant's square;
  * the values of `means2D` are ignored (as upstream, it only receives a gradient: (dL/dpx 0.5 W, dL/dpy 0.5 H, 0));
  * `prefiltered` and `debug` are accepted and unused.
There is no CPU compute path: a host tensor is refused.
"""
from __future__ import annotations

import ctypes as C
import os
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


class _Workspace:
    """A pixie_raster_forward workspace and what it was sized for.  A GaussianRasterizer keeps one between its forward-only calls; a
    differentiable render gets one of its own, which belongs to that render's autograd node, because the backward reads it as the
    forward left it and the module's is overwritten by the next call."""

    def __init__(self):
        self._workspace = None
        self._capacity = 0             # instances the workspace was sized for
        self._key = None


def _one_of_shs_or_colors(shs, colors_precomp):
    if (shs is None) == (colors_precomp is None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')     # the reference's text, as callers may match it


def _check_output(t, shape, dtype, device, message):
    if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise ValueError(message)


def _to_rgb8(images):
    """float images with values in [0, 1] as 8 bits: round(clip(255 x, 0, 255))"""
    return (images.detach().float() * 255.0).clamp(0.0, 255.0).round().to(torch.uint8)


def _ensure_workspace(holder, lib, n, W, H, device, instances):
    key = (n, W, H, device)
    if holder._workspace is not None and holder._key == key and holder._capacity >= instances:
        return
    need = lib.pixie_raster_workspace_bytes(n, W, H, int(instances))
    if need < 0:
        _lib.check(1, "pixie_raster_workspace_bytes", lib=lib)
    holder._workspace = torch.empty((max(int(need), 16),), dtype=torch.uint8, device=device)
    holder._capacity, holder._key = int(instances), key


_GRAD_INPUTS = ("means3D", "means2D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp")


class _Rasterize(torch.autograd.Function):
    """The differentiable render: forward = GaussianRasterizer._render on a workspace of its own, backward = one pixie_raster_backward
    call on the current stream.  Not differentiable twice."""

    @staticmethod
    def forward(ctx, rasterizer, aux, *inputs):
        given = dict(zip(_GRAD_INPUTS, inputs))
        out, radii, final_T, n_contrib, state = rasterizer._render(_Workspace(), True, given["means3D"], given["opacities"], given["shs"],
                                                                   given["colors_precomp"], given["scales"], given["rotations"], given["cov3D_precomp"],
                                                                   None, True)
        ctx.state = state                      # descriptor, workspace, instance count, SH parameters
        ctx.meta = [None if t is None else (tuple(t.shape), t.dtype) for t in inputs]
        ctx.save_for_backward(out, radii, final_T, n_contrib, *state["tensors"])
        ctx.mark_non_differentiable(radii, final_T, n_contrib)
        return out, radii, final_T, n_contrib

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_radii, g_final_T, g_n_contrib):
        none = (None,) * (2 + len(_GRAD_INPUTS))
        if g_out is None:
            return none
        st = ctx.state
        saved = ctx.saved_tensors              # raises if one of them was modified in place since the forward
        out = saved[0]
        device, n = out.device, st["n"]
        need = dict(zip(_GRAD_INPUTS, ctx.needs_input_grad[2:]))
        shapes = {"means3D": (n, 3), "means2D": (n, 3), "opacities": (n,), "shs": (n, st["sh_k"], 3), "colors_precomp": (n, 3),
                  "scales": (n, 3), "rotations": (n, 4), "cov3D_precomp": (n, 6)}
        grads = {k: torch.empty(shapes[k], dtype=torch.float32, device=device) for k in _GRAD_INPUTS if need[k]}
        g_out = g_out.detach().to(torch.float32).contiguous()
        lib = _lib.load()
        b = _lib.RasterBackwardDesc()
        b.forward = st["desc"]
        b.instances = st["instances"]
        if st["shs"] is not None:
            b.d_shs, b.sh_k, b.sh_degree = _ptr(st["shs"]), st["sh_k"], st["sh_degree"]
            b.campos = (C.c_float * 3)(*st["campos"])
        b.d_dL_dcolor = g_out.data_ptr()
        for field, key in (("d_dL_dmeans3D", "means3D"), ("d_dL_dmeans2D", "means2D"), ("d_dL_dopacity", "opacities"), ("d_dL_dshs", "shs"),
                           ("d_dL_dcolors", "colors_precomp"), ("d_dL_dscales", "scales"), ("d_dL_drotations", "rotations"),
                           ("d_dL_dcov3D", "cov3D_precomp")):
            setattr(b, field, _ptr(grads.get(key)))
        with torch.cuda.device(device):
            nb = lib.pixie_raster_backward_workspace_bytes(n, st["W"], st["H"], st["instances"])
            if nb < 0:
                _lib.check(1, "pixie_raster_backward_workspace_bytes", lib=lib)
            gws = torch.empty((max(int(nb), 16),), dtype=torch.uint8, device=device)
            b.d_grad_workspace, b.grad_workspace_bytes = gws.data_ptr(), gws.numel()
            rc = lib.pixie_raster_backward(C.byref(b), _lib.current_stream_ptr())
        _lib.check(rc, "pixie_raster_backward", lib=lib)
        result = []
        for k, meta in zip(_GRAD_INPUTS, ctx.meta):
            g = grads.get(k)
            result.append(None if g is None or meta is None else g.reshape(meta[0]).to(meta[1]))
        return (None, None) + tuple(result)


class GaussianRasterizer(torch.nn.Module):
    """`GaussianRasterizer(raster_settings)(means3D, means2D, opacities, ...)` -> (color (3, H, W), radii (N,) int32).
    The workspace is kept between calls and grows when a render needs more instances (Gaussian-tile pairs) than it holds.
    After a call, `last_instances` is that render's instance count; `forward(..., aux=True)` also returns (final_T, n_contrib).

    With grad mode on, an input among means3D, means2D, opacities, shs / colors_precomp, scales / rotations / cov3D_precomp that requires
    grad, and no `out=`, the colour is differentiable with respect to those inputs (radii, final_T and n_contrib are not; neither are
    the camera matrices; double backward is not supported).  Such a render runs on a workspace owned by its autograd node, so any
    number of renders may be outstanding before their backwards run, in any order.  Otherwise the call is the forward-only render:
    same workspace reuse, same launches, same bits as before."""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings
        self._ws = _Workspace()        # of the forward-only calls
        self._host = None              # (settings object, viewmatrix, projmatrix, bg as ctypes arrays): read back once per settings
        self.last_instances = 0
        self._owned_hint = (None, 0)   # (shape key, instance capacity) of the last differentiable render

    _workspace = property(lambda self: self._ws._workspace)
    _capacity = property(lambda self: self._ws._capacity)

    def _ensure_workspace(self, lib, n, device, instances):
        s = self.raster_settings
        _ensure_workspace(self._ws, lib, n, int(s.image_width), int(s.image_height), device, instances)

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
        _one_of_shs_or_colors(shs, colors_precomp)
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        inputs = (means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp)
        if out is None and torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in inputs):
            color, radii, final_T, n_contrib = _Rasterize.apply(self, aux, *inputs)
            return (color, radii, final_T, n_contrib) if aux else (color, radii)
        res = self._render(self._ws, False, means3D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp, out, aux)
        return res[:4] if aux else res[:2]

    def _render(self, holder, differentiable, means3D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp, out, aux):
        """One pixie_raster_forward on the workspace `holder`: the module's own, or with `differentiable` the one that render's
        autograd node will own.  Returns (out, radii, final_T, n_contrib, what a backward needs: None unless `differentiable`)."""
        s = self.raster_settings
        means = _device_f32(means3D, "GaussianRasterizer: means3D", (3,))
        n, device = means.shape[0], means.device
        sh = None
        if shs is not None:
            colors = sh_to_rgb(shs, int(s.sh_degree), means, self._host_settings()[4])
            if differentiable:
                sh = _device_f32(shs, "GaussianRasterizer: shs", tuple(shs.shape[1:]), n)
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
        else:
            _check_output(out, (3, H, W), torch.float32, device, f"GaussianRasterizer: out must be a contiguous float32 (3, {H}, {W}) tensor on {device}")
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
            same = self._ws._key == (n, W, H, device)
            guess = self._capacity if same else 4 * n      # a first guess: four tiles per Gaussian
            if differentiable and self._owned_hint[0] == (n, W, H, device):
                guess = max(guess, self._owned_hint[1])    # what the last differentiable render of this shape needed
            _ensure_workspace(holder, lib, n, W, H, device, guess)
            for attempt in (0, 1):
                d.d_workspace, d.workspace_bytes = holder._workspace.data_ptr(), holder._workspace.numel()
                rc = lib.pixie_raster_forward(C.byref(d), C.byref(count), _lib.current_stream_ptr())
                if rc == 0 or attempt == 1 or count.value <= 0:
                    break
                # Too small?  Decided in bytes, not instances: the library's sort storage need not grow monotonically with the count.
                grown = count.value + count.value // 2
                need = max(lib.pixie_raster_workspace_bytes(n, W, H, count.value), lib.pixie_raster_workspace_bytes(n, W, H, grown))
                if need <= holder._workspace.numel():
                    break                                  # the call failed for another reason: report it
                holder._workspace = torch.empty((int(need),), dtype=torch.uint8, device=device)      # grow to 1.5 x and retry once
                holder._capacity = grown
        _lib.check(rc, "pixie_raster_forward", lib=lib)
        self.last_instances = int(count.value)
        if not differentiable:
            return out, radii, final_T, n_contrib, None
        self._owned_hint = ((n, W, H, device), holder._capacity)
        state = dict(desc=d, instances=int(count.value), n=n, W=W, H=H, workspace=holder._workspace, shs=sh, sh_k=0 if sh is None else int(sh.shape[1]),
                     sh_degree=int(s.sh_degree), campos=[float(x) for x in self._host_settings()[4]],
                     tensors=[t for t in (means, opac, colors, cov, sc, rot, sh) if t is not None])
        return out, radii, final_T, n_contrib, state


def render_frames(frames, settings_per_frame, opacity, shs=None, colors_precomp=None, unselected=None, rasterizer=None, batch=None):
    """Renders what `SceneBatch.run_frames` returns for a scene -- (pos (F, N, 3), cov (F, N, 6), ...) -- into (F, 3, H, W) on the
    device; frame f equals `GaussianRasterizer(settings_f)(pos[f], None, opacity, shs or colors_precomp, cov3D_precomp=cov[f])` bit
    for bit.  `settings_per_frame`: one GaussianRasterizationSettings, or one per frame (a moving camera) with one image size.
    Exactly one of `shs` (N', K, 3; evaluated per frame at sh_degree from campos) and `colors_precomp` (N', 3).
    `unselected`: (pos (M, 3), cov (M, 6)) of Gaussians that do not simulate, appended to every frame (gs_simulation.py:602-606);
    `opacity` and the colours then cover N' = N + M Gaussians.
    `batch`: None renders frame by frame (a call, a colour launch and a stream synchronise per frame); True or a
    FrameBatchRasterizer hands the sequence to `render_frame_batch`, which gives the same images.
    Forward only: the frames carry no graph, whatever the inputs require."""
    if batch is not None and batch is not False:
        return render_frame_batch(frames, settings_per_frame, opacity, shs=shs, colors_precomp=colors_precomp, unselected=unselected,
                                  rasterizer=batch if isinstance(batch, FrameBatchRasterizer) else None)
    pos, cov = frames[0], frames[1]
    if cov is None:
        raise ValueError("render_frames: the frames carry no covariance (FrameSchedule.with_cov)")
    _one_of_shs_or_colors(shs, colors_precomp)
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


class FrameBatchOutput(NamedTuple):
    color: object          # (V, 3, H, W) float32, or None
    rgb8: object           # (V, H, W, 3) uint8, or None
    radii: object          # (V, N) int32
    final_T: object        # (V, H, W) float32, or None
    n_contrib: object      # (V, H, W) int32, or None


def _view_f32(t, what, n, tail):
    """`t` as a float32 device tensor (V, n, tail) whose views are dense, and the view stride in elements.  A tensor that already is
    one -- a slice of a larger (F, N, tail) tensor, or a view expanded with stride 0 -- is passed through without a copy."""
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise ValueError(f"{what} must be a tensor on a HIP device (there is no CPU path)")
    t = t.detach()
    if t.dim() != 3 or t.shape[1] != n or t.shape[2] != tail:
        raise ValueError(f"{what} must be (views, {n}, {tail}), got {tuple(t.shape)}")
    dense = t.dtype == torch.float32 and t.stride(0) >= 0 and (n <= 1 or t.stride(1) == tail) and t.stride(2) == 1
    if not dense:
        t = t.float().contiguous()
    return t, int(t.stride(0))


class FrameBatchRasterizer:
    """Renders V views of one Gaussian set -- a frame sequence -- in one pixie_raster_forward_batch call: one projection launch, one
    scan and one stream synchronise for the whole call, then one sort and one render launch per group of views.  The workspace is
    kept between calls.  Its instance capacity starts at four tiles per Gaussian-view, as far as `max_workspace_bytes` allows, and
    grows once when a single view needs more.  After a call `last_instances` holds the per-view instance counts and `last_groups`
    the number of sort groups.  Forward only: its outputs carry no graph (the differentiable render is `GaussianRasterizer`)."""

    def __init__(self, max_workspace_bytes=1 << 30):
        self.max_workspace_bytes = int(max_workspace_bytes)
        self._workspace = None
        self._capacity = 0
        self._key = None
        self._host = None              # (ids, settings kept alive, RasterView array, bg, scale_modifier, sh_degree, H, W)
        self.last_instances = []
        self.last_groups = 0

    def _host_views(self, settings):
        ids = tuple(id(s) for s in settings)
        if self._host is not None and self._host[0] == ids:
            return self._host
        first = settings[0]
        H, W = int(first.image_height), int(first.image_width)
        unique = {}
        for s in settings:
            unique.setdefault(id(s), s)
            if (int(s.image_height), int(s.image_width)) != (H, W):
                raise ValueError("FrameBatchRasterizer: every view must have the same image size")
            if float(s.scale_modifier) != float(first.scale_modifier) or int(s.sh_degree) != int(first.sh_degree):
                raise ValueError("FrameBatchRasterizer: every view must have the same scale_modifier and sh_degree")
        rows = []
        for s in unique.values():
            parts = []
            for name, count in (("viewmatrix", 16), ("projmatrix", 16), ("campos", 3), ("bg", 3)):
                v = torch.as_tensor(getattr(s, name)).detach().to(torch.float32).reshape(-1)
                if v.numel() != count:
                    raise ValueError(f"FrameBatchRasterizer: {name} must hold {count} values, got {v.numel()}")
                parts.append(v)
            if len({v.device for v in parts}) > 1:
                parts = [v.cpu() for v in parts]
            rows.append(torch.cat(parts))
        if len({r.device for r in rows}) > 1:
            rows = [r.cpu() for r in rows]
        host = torch.stack(rows).cpu()                 # every distinct camera of the call in one device-to-host copy
        row_of = {k: j for j, k in enumerate(unique)}
        table = torch.empty((len(settings), 37), dtype=torch.float32)
        for v, s in enumerate(settings):
            r = host[row_of[id(s)]]
            if not torch.equal(r[35:38], host[0, 35:38]):
                raise ValueError("FrameBatchRasterizer: every view must have the same background")
            table[v, :35] = r[:35]
            table[v, 35], table[v, 36] = float(s.tanfovx), float(s.tanfovy)
        views = (_lib.RasterView * len(settings)).from_buffer_copy(table.numpy().tobytes())
        self._host = (ids, list(settings), views, [float(x) for x in host[0, 35:38]], float(first.scale_modifier), int(first.sh_degree), H, W)
        return self._host

    def _workspace_bytes(self, lib, n, views, W, H, capacity):
        need = lib.pixie_raster_batch_workspace_bytes(n, views, W, H, int(capacity))
        if need < 0:
            _lib.check(1, "pixie_raster_batch_workspace_bytes", lib=lib)
        return int(need)

    def _ensure_workspace(self, lib, key, capacity, exact):
        if self._workspace is not None and self._key == key and (self._capacity == capacity if exact else self._capacity >= capacity):
            return
        need = self._workspace_bytes(lib, key[0], key[1], key[2], key[3], capacity)
        self._workspace = torch.empty((max(need, 16),), dtype=torch.uint8, device=key[4])
        self._capacity, self._key = int(capacity), key

    def _first_capacity(self, lib, n, views, W, H):
        one = min(4 * n, 0xFFFFFFFF)
        cap = min(one * views, 0xFFFFFFFF)
        while cap > one and self._workspace_bytes(lib, n, views, W, H, cap) > self.max_workspace_bytes:
            cap = max(cap // 2, one)
        return cap

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    def forward(self, means, cov3D, settings, opacities, shs=None, colors_precomp=None, static=None, out=None, out_rgb8=None, aux=False,
                capacity=None):
        """means (V, N, 3) and cov3D (V, N, 6) on a HIP device (views dense, any view stride: a slice of a longer sequence is not
        copied); `settings`: one GaussianRasterizationSettings or V of them with one image size, background, scale_modifier and
        sh_degree; `static`: (pos (M, 3), cov (M, 6)) appended to every view; `opacities` (N + M,); exactly one of `shs`
        (N + M, K, 3) and `colors_precomp` ((N + M, 3) shared, or (V, N + M, 3)).  `out`: a (V, 3, H, W) float32 tensor to fill, None
        to allocate one, False for none; `out_rgb8`: a (V, H, W, 3) uint8 tensor, True to allocate one, None for none.
        `capacity`: the instance capacity of one sort, instead of the rasteriser's own guess.  Returns a FrameBatchOutput."""
        _one_of_shs_or_colors(shs, colors_precomp)
        if not torch.is_tensor(means) or not torch.is_tensor(cov3D) or means.dim() != 3:
            raise ValueError("FrameBatchRasterizer: means3D and cov3D must be (views, N, 3) and (views, N, 6) tensors")
        V, n_dyn = int(means.shape[0]), int(means.shape[1])
        per_view = [settings] * V if isinstance(settings, GaussianRasterizationSettings) else list(settings)
        if len(per_view) != V:
            raise ValueError(f"FrameBatchRasterizer: {len(per_view)} settings for {V} views")
        if V < 1:
            raise ValueError("FrameBatchRasterizer: no view to render")
        means, means_stride = _view_f32(means, "FrameBatchRasterizer: means3D", n_dyn, 3)
        cov, cov_stride = _view_f32(cov3D, "FrameBatchRasterizer: cov3D", n_dyn, 6)
        device = means.device
        st_pos = st_cov = None
        if static is not None:
            st_pos = _device_f32(static[0], "FrameBatchRasterizer: static positions", (3,))
            st_cov = _device_f32(static[1], "FrameBatchRasterizer: static covariances", (6,), st_pos.shape[0])
        n_static = 0 if st_pos is None else int(st_pos.shape[0])
        n = n_dyn + n_static
        opac = _device_f32(opacities, "FrameBatchRasterizer: opacities", (), n)
        sh = colors = None
        colors_stride = 0
        if shs is not None:
            if not torch.is_tensor(shs) or shs.dim() != 3 or shs.shape[2] != 3:
                raise ValueError(f"FrameBatchRasterizer: shs must be (N, K, 3), got {tuple(shs.shape) if torch.is_tensor(shs) else type(shs)}")
            sh = _device_f32(shs, "FrameBatchRasterizer: shs", tuple(shs.shape[1:]), n)
        elif torch.is_tensor(colors_precomp) and colors_precomp.dim() == 3:
            if colors_precomp.shape[0] != V:
                raise ValueError(f"FrameBatchRasterizer: per-view colors_precomp must be ({V}, {n}, 3), got {tuple(colors_precomp.shape)}")
            colors, colors_stride = _view_f32(colors_precomp, "FrameBatchRasterizer: colors_precomp", n, 3)
        else:
            colors = _device_f32(colors_precomp, "FrameBatchRasterizer: colors_precomp", (3,), n)
        _, _, views, bg, scale_modifier, sh_degree, H, W = self._host_views(per_view)

        if out is None and (out_rgb8 is None or out_rgb8 is False):
            out = True
        if out is True:
            out = torch.empty((V, 3, H, W), dtype=torch.float32, device=device)
        elif out is None or out is False:
            out = None
        else:
            _check_output(out, (V, 3, H, W), torch.float32, device,
                          f"FrameBatchRasterizer: out must be a contiguous float32 ({V}, 3, {H}, {W}) tensor on {device}")
        if out_rgb8 is True:
            out_rgb8 = torch.empty((V, H, W, 3), dtype=torch.uint8, device=device)
        elif out_rgb8 is None or out_rgb8 is False:
            out_rgb8 = None
        else:
            _check_output(out_rgb8, (V, H, W, 3), torch.uint8, device,
                          f"FrameBatchRasterizer: out_rgb8 must be a contiguous uint8 ({V}, {H}, {W}, 3) tensor on {device}")
        radii = torch.empty((V, n), dtype=torch.int32, device=device)
        final_T = torch.empty((V, H, W), dtype=torch.float32, device=device) if aux else None
        n_contrib = torch.empty((V, H, W), dtype=torch.int32, device=device) if aux else None

        lib = _lib.load()
        d = _lib.RasterBatchDesc()
        d.views, d.n_dyn, d.n_static, d.width, d.height = V, n_dyn, n_static, W, H
        d.sh_degree, d.k_coeffs, d.scale_modifier = sh_degree, 0 if sh is None else int(sh.shape[1]), scale_modifier
        d.bg = (C.c_float * 3)(*bg)
        d.view = views
        d.means_view_stride, d.cov3d_view_stride, d.colors_view_stride = means_stride, cov_stride, colors_stride
        for name, t in (("d_means", means), ("d_cov3d", cov), ("d_static_means", st_pos), ("d_static_cov3d", st_cov), ("d_opacity", opac),
                        ("d_colors", colors), ("d_shs", sh), ("d_out_color", out), ("d_out_rgb8", out_rgb8), ("d_radii", radii),
                        ("d_final_T", final_T), ("d_n_contrib", n_contrib)):
            setattr(d, name, t.data_ptr() if t is not None and t.numel() else None)
        counts = (C.c_int64 * V)()
        groups = C.c_int32(0)
        key = (n, V, W, H, device)
        with torch.cuda.device(device):
            if capacity is not None:
                self._ensure_workspace(lib, key, int(capacity), exact=True)
            else:
                self._ensure_workspace(lib, key, self._capacity if self._key == key else self._first_capacity(lib, n, V, W, H), exact=False)
            for attempt in (0, 1):
                d.d_workspace, d.workspace_bytes, d.max_instances = self._workspace.data_ptr(), self._workspace.numel(), self._capacity
                rc = lib.pixie_raster_forward_batch(C.byref(d), counts, C.byref(groups), _lib.current_stream_ptr())
                largest = max(counts)
                if rc == 0 or attempt == 1 or largest <= self._capacity:
                    break                                  # done, or the call failed for another reason: report it
                self._ensure_workspace(lib, key, min(largest + largest // 2, 0xFFFFFFFF), exact=True)    # one view did not fit: grow once
        _lib.check(rc, "pixie_raster_forward_batch", lib=lib)
        self.last_instances = [int(c) for c in counts]
        self.last_groups = int(groups.value)
        return FrameBatchOutput(out, out_rgb8, radii, final_T, n_contrib)


def _default_frames_per_call(n, n_frames, max_workspace_bytes):
    """As many frames as keep the part of the workspace sized by views x N (60 bytes per Gaussian-view) within half of
    `max_workspace_bytes`, and views x N within one scan."""
    per_view = max(60 * n, 1)
    fit = max(max_workspace_bytes // 2 // per_view, 1)
    scan = max((2 ** 31 - 2) // max(n, 1), 1)
    return int(max(1, min(n_frames, fit, scan, 65535)))


def render_frame_batch(frames, settings_per_frame, opacity, shs=None, colors_precomp=None, unselected=None, frames_per_call=None, out=None,
                       out_rgb8=None, rasterizer=None):
    """`render_frames` through FrameBatchRasterizer: the frames `SceneBatch.run_frames` returns for a scene -- (pos (F, N, 3),
    cov (F, N, 6), ...) -- go to the rasteriser as they lie on the device, `frames_per_call` at a time (default: what keeps the
    workspace's fixed part within half of the rasteriser's `max_workspace_bytes`), with one stream synchronise per call instead of
    one per frame, and without the per-frame concatenation of `unselected`.  Same arguments and argument errors as `render_frames`.
    Returns (F, 3, H, W) float32, bit for bit what `render_frames` gives; `out` fills a given tensor.  `out_rgb8` (True, or a
    (F, H, W, 3) uint8 tensor) also writes the 8-bit frames `save_frame_png` would; asked for alone, it is what is returned.
    Forward only, like `render_frames`."""
    pos, cov = frames[0], frames[1]
    if cov is None:
        raise ValueError("render_frame_batch: the frames carry no covariance (FrameSchedule.with_cov)")
    _one_of_shs_or_colors(shs, colors_precomp)
    n_frames = int(pos.shape[0])
    per_frame = [settings_per_frame] * n_frames if isinstance(settings_per_frame, GaussianRasterizationSettings) else list(settings_per_frame)
    if len(per_frame) != n_frames:
        raise ValueError(f"render_frame_batch: {len(per_frame)} settings for {n_frames} frames")
    if not torch.is_tensor(pos) or pos.device.type != "cuda":
        raise ValueError("render_frame_batch: frames must be tensors on a HIP device (there is no CPU path)")
    if n_frames == 0:
        raise ValueError("render_frame_batch: no frame to render")
    H, W = int(per_frame[0].image_height), int(per_frame[0].image_width)
    only_rgb8 = out is None and out_rgb8 is not None and out_rgb8 is not False
    if out is None and not only_rgb8:
        out = torch.empty((n_frames, 3, H, W), dtype=torch.float32, device=pos.device)
    if out_rgb8 is True:
        out_rgb8 = torch.empty((n_frames, H, W, 3), dtype=torch.uint8, device=pos.device)
    elif out_rgb8 is False:
        out_rgb8 = None
    for t, shape, dtype in ((out, (n_frames, 3, H, W), torch.float32), (out_rgb8, (n_frames, H, W, 3), torch.uint8)):
        if t is not None:
            _check_output(t, shape, dtype, pos.device, f"render_frame_batch: an output must be a contiguous {dtype} {shape} tensor on {pos.device}")
    r = rasterizer if rasterizer is not None else FrameBatchRasterizer()
    n = int(pos.shape[1]) + (0 if unselected is None else int(unselected[0].shape[0]))
    step = int(frames_per_call) if frames_per_call else _default_frames_per_call(n, n_frames, r.max_workspace_bytes)
    if step < 1:
        raise ValueError(f"render_frame_batch: frames_per_call {frames_per_call} must be positive")
    per_view_colors = colors_precomp is not None and torch.is_tensor(colors_precomp) and colors_precomp.dim() == 3
    instances, groups = [], 0
    for f0 in range(0, n_frames, step):
        f1 = min(f0 + step, n_frames)
        r(pos[f0:f1], cov[f0:f1], per_frame[f0:f1], opacity, shs=shs, colors_precomp=colors_precomp[f0:f1] if per_view_colors else colors_precomp,
          static=unselected, out=False if out is None else out[f0:f1], out_rgb8=None if out_rgb8 is None else out_rgb8[f0:f1])
        instances += r.last_instances
        groups += r.last_groups
    r.last_instances, r.last_groups = instances, groups          # of the whole sequence
    return out_rgb8 if only_rgb8 else out


def save_frame_png(path, image):
    """Writes a (3, H, W) RGB image with values in [0, 1] as an 8-bit PNG: round(clip(255 x, 0, 255)), the file the reference's
    cvtColor + imwrite pair produces for frames/%05d.png.  Returns the path."""
    if not torch.is_tensor(image) or image.dim() != 3 or image.shape[0] != 3:
        raise ValueError("save_frame_png: image must be a (3, H, W) tensor")
    try:
        from PIL import Image
    except ImportError as exc:
        raise RuntimeError("save_frame_png needs Pillow (PIL), which is not installed") from exc
    a = _to_rgb8(image).permute(1, 2, 0).contiguous().cpu().numpy()
    Image.fromarray(a).save(path, format="PNG")
    return path


def save_frame_pngs(dir, rgb8_or_images, start=0):
    """Writes frames as `dir`/%05d.png from number `start`: a (F, H, W, 3) uint8 tensor as `render_frame_batch(out_rgb8=...)`
    gives it, or (F, 3, H, W) float images, which are converted as `save_frame_png` converts one.  One device-to-host copy for the
    whole sequence.  Returns the paths."""
    t = rgb8_or_images
    if not torch.is_tensor(t) or t.dim() != 4 or not ((t.dtype == torch.uint8 and t.shape[3] == 3) or (t.is_floating_point() and t.shape[1] == 3)):
        raise ValueError("save_frame_pngs: frames must be a (F, H, W, 3) uint8 or a (F, 3, H, W) floating-point tensor")
    try:
        from PIL import Image
    except ImportError as exc:
        raise RuntimeError("save_frame_png needs Pillow (PIL), which is not installed") from exc
    if t.dtype != torch.uint8:
        t = _to_rgb8(t).permute(0, 2, 3, 1)
    a = t.detach().contiguous().cpu().numpy()
    os.makedirs(dir, exist_ok=True)
    paths = []
    for f in range(a.shape[0]):
        paths.append(os.path.join(dir, "%05d.png" % (start + f)))
        Image.fromarray(a[f]).save(paths[-1], format="PNG")
    return paths
