"""What gaussian-splatting/train.py does with the gradients of one iteration, on the device in HIP (pixie_amd/csrc/gs_optim.hip).

    GaussianAdam(params, lr=0.0, betas=(0.9, 0.999), eps=1e-15)      gaussians.optimizer (scene/gaussian_model.py:163)
    add_densification_stats(accum, denom, max_radii2D, grad, radii)  train.py:114-116
    densify_and_prune(gaussians, max_grad, min_opacity, extent, max_screen_size)   gaussian_model.py:393-405
    reset_opacity(gaussians)                                         gaussian_model.py:210-213

`GaussianAdam` is a `torch.optim.Optimizer` with torch Adam's state keys (`step`, `exp_avg`, `exp_avg_sq`) and `param_groups`
layout, so the reference's optimiser surgery (`replace_tensor_to_optimizer`, `_prune_optimizer`, `cat_tensors_to_optimizer`),
`update_learning_rate` and checkpoints (`optimizer.state_dict()`) work on it unmodified, and a `torch.optim.Adam` state dict loads
into it and the reverse.  `step()` is ONE kernel launch for all groups; the update is dense (a Gaussian with a zero gradient still
moves on its momentum, as in the reference).  There is no CPU compute path: `step()` refuses a host parameter.

`densify_and_prune` is plan (classify, scan, the call's only synchronise), a draw of the split's noise, and one emit launch that
writes the six parameters, their twelve Adam moments, an int32 `source_index` per output row and the three zeroed statistics arrays
at their final size.  Output rows are in the reference's order: originals that were not split, clones, first split children, second
split children, each in source order, filtered by the final prune.

Differences from the reference: the split's noise is `torch.randn((2 n_split, 3))`, the same distribution as its `torch.normal`
but another stream of the generator; the prune term `max_radii2D > max_screen_size`, which can never fire there because
`densification_postfix` zeroes `max_radii2D` first, is not evaluated; `torch.cuda.empty_cache()` is not called.
"""
from __future__ import annotations

import ctypes as C
import inspect
import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch
from torch import nn

from . import _lib

FIELDS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")     # the reference's group names, in its order
_ROW = {"xyz": 3, "f_dc": 3, "opacity": 1, "scaling": 3, "rotation": 4}    # floats per row; f_rest: 3 ((sh_degree + 1)^2 - 1)
MAX_GROUPS_PER_LAUNCH = 8


def _adam_defaults(lr, betas, eps):
    """torch.optim.Adam's own defaults (whatever this torch version has), so that either optimiser loads the other's state dict"""
    d = {}
    for name, par in inspect.signature(torch.optim.Adam.__init__).parameters.items():
        if name in ("self", "params") or par.default is inspect.Parameter.empty:
            continue
        d[name] = par.default
    d.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False)
    return d


class GaussianAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=0.0, betas=(0.9, 0.999), eps=1e-15, weight_decay=0, amsgrad=False, maximize=False):
        if not 0.0 <= lr:
            raise ValueError(f"GaussianAdam: invalid learning rate {lr}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"GaussianAdam: invalid betas {betas}")
        if not 0.0 <= eps:
            raise ValueError(f"GaussianAdam: invalid eps {eps}")
        defaults = _adam_defaults(lr, betas, eps)
        defaults.update(weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        super().__init__(params, defaults)
        for i, group in enumerate(self.param_groups):
            self._check_group(i, group, need_device=False)

    @staticmethod
    def _check_group(i, group, need_device=True):
        name = group.get("name", i)
        if group.get("weight_decay", 0) != 0:
            raise ValueError(f"GaussianAdam: group {name!r} has weight decay {group['weight_decay']}; weight decay is not supported")
        if group.get("amsgrad", False):
            raise ValueError(f"GaussianAdam: group {name!r} asks for amsgrad, which is not supported")
        if group.get("maximize", False):
            raise ValueError(f"GaussianAdam: group {name!r} asks for maximize, which is not supported")
        if len(group["params"]) != 1:
            raise ValueError(f"GaussianAdam: group {name!r} has {len(group['params'])} tensors; every group holds exactly one tensor")
        p = group["params"][0]
        if p.dtype != torch.float32:
            raise ValueError(f"GaussianAdam: the parameter of group {name!r} is {p.dtype}, not float32")
        if not p.is_contiguous():
            raise ValueError(f"GaussianAdam: the parameter of group {name!r} is not contiguous")
        if need_device and p.device.type != "cuda":
            raise ValueError(f"GaussianAdam: the parameter of group {name!r} is a host tensor on {p.device} (there is no CPU path)")

    @staticmethod
    def init_state(p):
        """the state torch.optim.Adam creates for a parameter on its first step"""
        return {"step": torch.tensor(0.0, dtype=torch.float32),
                "exp_avg": torch.zeros_like(p, memory_format=torch.preserve_format),
                "exp_avg_sq": torch.zeros_like(p, memory_format=torch.preserve_format)}

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []          # (parameter, gradient, exp_avg, exp_avg_sq, step_size, bias_correction2_sqrt, betas, eps)
        for i, group in enumerate(self.param_groups):
            self._check_group(i, group)
            p = group["params"][0]
            if p.grad is None:
                continue
            g = p.grad
            name = group.get("name", i)
            if g.is_sparse:
                raise ValueError(f"GaussianAdam: the gradient of group {name!r} is sparse")
            if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                raise ValueError(f"GaussianAdam: the gradient of group {name!r} is {g.dtype} {tuple(g.shape)} on {g.device}, "
                                 f"not float32 {tuple(p.shape)} on {p.device}")
            if not g.is_contiguous():
                g = g.contiguous()
            state = self.state[p]
            if len(state) == 0:
                state.update(self.init_state(p))
            for key in ("exp_avg", "exp_avg_sq"):
                m = state[key]
                if m.dtype != torch.float32 or m.device != p.device or m.shape != p.shape or not m.is_contiguous():
                    raise ValueError(f"GaussianAdam: state {key!r} of group {name!r} is {m.dtype} {tuple(m.shape)} on {m.device} "
                                     f"(contiguous: {m.is_contiguous()}), not contiguous float32 {tuple(p.shape)} on {p.device}")
            if torch.is_tensor(state["step"]):
                state["step"] += 1
                t = float(state["step"])
            else:
                state["step"] = t = state["step"] + 1
            beta1, beta2 = group["betas"]
            # as torch.optim.Adam: in double, rounded once when it reaches the kernel
            step_size = group["lr"] / (1 - beta1 ** t)
            bc2_sqrt = (1 - beta2 ** t) ** 0.5
            work.append((p, g, state["exp_avg"], state["exp_avg_sq"], step_size, bc2_sqrt, (beta1, beta2), group["eps"]))
        if not work:
            return loss
        if any(w[6] != work[0][6] or w[7] != work[0][7] or w[0].device != work[0][0].device for w in work):
            raise ValueError("GaussianAdam: all groups must share betas, eps and the device (one launch takes one set)")
        lib = _lib.load()
        with torch.cuda.device(work[0][0].device):
            stream = _lib.current_stream_ptr()
            for k0 in range(0, len(work), MAX_GROUPS_PER_LAUNCH):
                chunk = work[k0:k0 + MAX_GROUPS_PER_LAUNCH]
                desc = _lib.GsAdamDesc()
                desc.beta1, desc.beta2 = chunk[0][6]
                desc.eps = chunk[0][7]
                desc.n_groups = len(chunk)
                for k, (p, g, m, v, step_size, bc2_sqrt, _, _) in enumerate(chunk):
                    grp = desc.group[k]
                    grp.param, grp.grad, grp.exp_avg, grp.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                    grp.count = p.numel()
                    grp.step_size = step_size
                    grp.bias_correction2_sqrt = bc2_sqrt
                _lib.check(lib.pixie_gs_adam_step(C.byref(desc), stream), "pixie_gs_adam_step", lib=lib)
        return loss


def _device_f32(t, name, shape=None):
    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise ValueError(f"{name} must be a tensor on a HIP device (there is no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be {tuple(shape)}, got {tuple(t.shape)}")
    return t


def add_densification_stats(xyz_gradient_accum, denom, max_radii2D, viewspace_grad, radii):
    """train.py:114-116 in one launch and without a synchronise: for every Gaussian with radii > 0,
    max_radii2D = max(max_radii2D, radii); xyz_gradient_accum += |viewspace_grad[:, :2]|; denom += 1.  All in place.
    xyz_gradient_accum, denom: (N, 1); max_radii2D: (N,); viewspace_grad: (N, 3); radii: (N,) int32, as the rasteriser returns it."""
    n = int(max_radii2D.shape[0])
    _device_f32(xyz_gradient_accum, "xyz_gradient_accum", (n, 1))
    _device_f32(denom, "denom", (n, 1))
    _device_f32(max_radii2D, "max_radii2D", (n,))
    _device_f32(viewspace_grad, "viewspace_grad", (n, 3))
    if not torch.is_tensor(radii) or radii.device != max_radii2D.device or radii.dtype != torch.int32 or tuple(radii.shape) != (n,) \
            or not radii.is_contiguous():
        raise ValueError(f"radii must be a contiguous int32 ({n},) tensor on {max_radii2D.device}")
    if n == 0:
        return
    lib = _lib.load()
    with torch.cuda.device(max_radii2D.device):
        rc = lib.pixie_gs_densify_stats(C.c_void_p(radii.data_ptr()), C.c_void_p(viewspace_grad.data_ptr()), n,
                                        C.c_void_p(max_radii2D.data_ptr()), C.c_void_p(xyz_gradient_accum.data_ptr()),
                                        C.c_void_p(denom.data_ptr()), _lib.current_stream_ptr())
        _lib.check(rc, "pixie_gs_densify_stats", lib=lib)


@dataclass
class DensifyResult:
    params: Dict[str, torch.Tensor]
    exp_avg: Dict[str, torch.Tensor]
    exp_avg_sq: Dict[str, torch.Tensor]
    xyz_gradient_accum: torch.Tensor
    denom: torch.Tensor
    max_radii2D: torch.Tensor
    source_index: torch.Tensor           # (M,) int32: the input row of every output row
    n_kept: int                          # originals that stay (not split, not pruned)
    n_cloned: int                        # clones that stay
    n_split_children: int                # split children that stay
    n_pruned: int                        # rows the final prune removed (originals, clones and children)
    n_split: int                         # Gaussians that were split


def _ptr_array(tensors):
    arr = (C.c_void_p * 6)()
    for k, t in enumerate(tensors):
        arr[k] = t.data_ptr() if t is not None and t.numel() > 0 else None
    return arr


def densify_and_prune_tensors(params, exp_avg, exp_avg_sq, xyz_gradient_accum, denom, max_grad, min_opacity, extent, percent_dense,
                              max_screen_size, noise=None, generator=None) -> DensifyResult:
    """The functional form: `params`, `exp_avg`, `exp_avg_sq` are dicts keyed by FIELDS (a moment may be None: no optimiser
    state yet, zeros); returns new tensors and leaves the inputs untouched.  `noise`: standard-normal (2 n_split, 3), row
    copy * n_split + (rank among the split Gaussians), as the reference's torch.normal lays out its draw."""
    xyz = params["xyz"]
    n = int(xyz.shape[0])
    dev = xyz.device
    shapes = {}
    for f in FIELDS:
        t = _device_f32(params[f], f"parameter {f!r}")
        if t.device != dev or t.shape[0] != n:
            raise ValueError(f"parameter {f!r} is {tuple(t.shape)} on {t.device}; expected {n} rows on {dev}")
        row = t.numel() // n if n else 0
        if f != "f_rest" and n and row != _ROW[f]:
            raise ValueError(f"parameter {f!r} has {row} floats per row, expected {_ROW[f]}")
        shapes[f] = tuple(t.shape[1:])
        for nm, mom in (("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            m = (mom or {}).get(f)
            if m is not None:
                _device_f32(m, f"{nm}[{f!r}]", t.shape)
    _device_f32(xyz_gradient_accum, "xyz_gradient_accum", (n, 1))
    _device_f32(denom, "denom", (n, 1))
    n_rest = params["f_rest"].numel() // n if n else 0

    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = _lib.current_stream_ptr()
        need = lib.pixie_gs_densify_workspace_bytes(n)
        if need < 0:
            _lib.check(1, "pixie_gs_densify_workspace_bytes", lib=lib)
        workspace = torch.empty((max(int(need), 16),), dtype=torch.uint8, device=dev)
        desc = _lib.GsDensifyDesc()
        desc.n, desc.n_rest, desc.has_max_screen_size = n, n_rest, 1 if max_screen_size else 0
        desc.max_grad, desc.min_opacity, desc.extent, desc.percent_dense = float(max_grad), float(min_opacity), float(extent), float(percent_dense)
        desc.d_xyz_gradient_accum, desc.d_denom = xyz_gradient_accum.data_ptr(), denom.data_ptr()
        desc.d_param = _ptr_array([params[f] for f in FIELDS])
        desc.d_exp_avg = _ptr_array([(exp_avg or {}).get(f) for f in FIELDS])
        desc.d_exp_avg_sq = _ptr_array([(exp_avg_sq or {}).get(f) for f in FIELDS])
        desc.d_workspace, desc.workspace_bytes = workspace.data_ptr(), workspace.numel()
        counts = (C.c_int64 * 4)()
        n_split_c = (C.c_int64 * 1)()
        rc = lib.pixie_gs_densify_plan(C.byref(desc), counts, n_split_c, stream)
        if rc in (_lib.GS_DENSIFY_BAD_MAX_GRAD, _lib.GS_DENSIFY_TOO_MANY_ROWS, _lib.GS_DENSIFY_EMPTY):
            raise ValueError(lib.pixie_last_error().decode())
        _lib.check(rc, "pixie_gs_densify_plan", lib=lib)
        n_kept, n_cloned, n_children, n_pruned = (int(c) for c in counts)
        n_split = int(n_split_c[0])
        m_rows = n_kept + n_cloned + n_children

        if noise is None:
            gen_dev = generator.device if generator is not None else dev
            noise = torch.randn((2 * n_split, 3), generator=generator, device=gen_dev, dtype=torch.float32).to(dev)
        else:
            _device_f32(noise, "noise", (2 * n_split, 3))

        def new(shape, dtype=torch.float32):
            return torch.empty(shape, dtype=dtype, device=dev)
        out_p = {f: new((m_rows,) + shapes[f]) for f in FIELDS}
        out_m = {f: new((m_rows,) + shapes[f]) for f in FIELDS}
        out_v = {f: new((m_rows,) + shapes[f]) for f in FIELDS}
        source_index = new((m_rows,), torch.int32)
        out_accum, out_denom, out_radii = new((m_rows, 1)), new((m_rows, 1)), new((m_rows,))
        outs = _lib.GsDensifyOuts()
        outs.n_out, outs.n_split = m_rows, n_split
        outs.d_noise = noise.data_ptr() if n_split else None
        outs.d_param = _ptr_array([out_p[f] for f in FIELDS])
        outs.d_exp_avg = _ptr_array([out_m[f] for f in FIELDS])
        outs.d_exp_avg_sq = _ptr_array([out_v[f] for f in FIELDS])
        outs.d_source_index = source_index.data_ptr() if m_rows else None
        outs.d_xyz_gradient_accum = out_accum.data_ptr() if m_rows else None
        outs.d_denom = out_denom.data_ptr() if m_rows else None
        outs.d_max_radii2D = out_radii.data_ptr() if m_rows else None
        _lib.check(lib.pixie_gs_densify_emit(C.byref(desc), C.byref(outs), stream), "pixie_gs_densify_emit", lib=lib)
        # workspace and noise go back to torch's caching allocator here; launches queued on this stream are ordered before any reuse
    return DensifyResult(out_p, out_m, out_v, out_accum, out_denom, out_radii, source_index, n_kept, n_cloned, n_children, n_pruned, n_split)


_ATTR = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation"}


def _groups_by_name(optimizer):
    groups = {g.get("name"): g for g in optimizer.param_groups}
    missing = [f for f in FIELDS if f not in groups]
    if missing:
        raise ValueError(f"the optimiser has no parameter group named {missing}")
    for f in FIELDS:
        if len(groups[f]["params"]) != 1:
            raise ValueError(f"group {f!r} has {len(groups[f]['params'])} tensors; every group holds exactly one tensor")
    return groups


def densify_and_prune(gaussians, max_grad, min_opacity, extent, max_screen_size, noise=None, generator=None) -> DensifyResult:
    """GaussianModel.densify_and_prune on any object with the reference model's attributes (_xyz, _features_dc, _features_rest,
    _opacity, _scaling, _rotation, optimizer, xyz_gradient_accum, denom, max_radii2D, percent_dense).  The new nn.Parameters and
    moments are installed into the optimiser the way the reference does it: the state dict object of each parameter is kept
    (so `step` is), re-keyed to the new parameter."""
    opt = gaussians.optimizer
    groups = _groups_by_name(opt)
    params, exp_avg, exp_avg_sq = {}, {}, {}
    for f in FIELDS:
        p = groups[f]["params"][0]
        if p is not getattr(gaussians, _ATTR[f]):
            raise ValueError(f"gaussians.{_ATTR[f]} is not the tensor of the optimiser's group {f!r}")
        st = opt.state.get(p, None)
        params[f] = p.detach()
        exp_avg[f] = st["exp_avg"] if st else None
        exp_avg_sq[f] = st["exp_avg_sq"] if st else None
    res = densify_and_prune_tensors(params, exp_avg, exp_avg_sq, gaussians.xyz_gradient_accum, gaussians.denom, max_grad, min_opacity,
                                    extent, gaussians.percent_dense, max_screen_size, noise=noise, generator=generator)
    for f in FIELDS:
        group = groups[f]
        old = group["params"][0]
        stored_state = opt.state.get(old, None)
        new = nn.Parameter(res.params[f].requires_grad_(True))
        if stored_state:
            stored_state["exp_avg"] = res.exp_avg[f]
            stored_state["exp_avg_sq"] = res.exp_avg_sq[f]
            del opt.state[old]
            opt.state[new] = stored_state
        group["params"][0] = new
        setattr(gaussians, _ATTR[f], new)
        res.params[f] = new
    gaussians.xyz_gradient_accum = res.xyz_gradient_accum
    gaussians.denom = res.denom
    gaussians.max_radii2D = res.max_radii2D
    return res


def reset_opacity(gaussians):
    """GaussianModel.reset_opacity: opacity = inverse_sigmoid(min(sigmoid(opacity), 0.01)), its two moments zeroed, `step` kept."""
    opt = gaussians.optimizer
    group = _groups_by_name(opt)["opacity"]
    old = group["params"][0]
    with torch.no_grad():
        x = torch.min(torch.sigmoid(old), torch.ones_like(old) * 0.01)
        value = torch.log(x / (1 - x))
    stored_state = opt.state.get(old, None)
    new = nn.Parameter(value.requires_grad_(True))
    if stored_state:
        stored_state["exp_avg"] = torch.zeros_like(value)
        stored_state["exp_avg_sq"] = torch.zeros_like(value)
        del opt.state[old]
        opt.state[new] = stored_state
    group["params"][0] = new
    gaussians._opacity = new
    return new
