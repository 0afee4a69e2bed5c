"""Proposal density fields on the device: nerfstudio's HashMLPDensityField (fields/density_fields.py) as one fused, differentiable launch.

nerfacto builds two of these (nerfacto.py:94-98: 5 hash levels x 2 features, 16 -> 128 / 256, 2^17 rows per level, ONE hidden layer of
16, one output, trunc_exp) and ProposalNetworkSampler.generate_ray_samples (pixie_amd/ray_sampling.py) calls `density_fn` once per
proposal level: at 4096 rays 1.44 M points per step, more than every other network of the model together.  field_query.HashMLP is 64
wide; this module is the 16-wide path over pixie_amd/csrc/density_field.hip: positions in the nerf frame -> contraction or
aabb -> selector -> hash grid -> 16-wide ReLU layers -> average_init_density * exp(h) * selector, with gradients for the hash table,
the weights and the biases under torch.autograd.

    HashMLPDensityField(aabb, num_layers, hidden_dim, spatial_distortion, use_linear, num_levels, max_res, base_res,
                        log2_hashmap_size, features_per_level, average_init_density, implementation)
    .density_fn(positions (..., 3)) -> (..., 1)         what ProposalNetworkSampler calls
    .get_density(ray_samples) -> (density, None)
    .from_nerfstudio_state_dict / .from_tcnn_params     the reference's two parameter layouts
    .to_trainable_hashmlp()                             the zero-padded 64-wide twin (field_training.TrainableHashMLP), for tests and benchmarks

Under torch.no_grad(), or when nothing requires a gradient, forward launches the inference kernel and saves nothing (the sampler
takes this path on four steps out of five).  Otherwise the autograd.Function saves the positions and references to the parameters (no copies:
the backward recomputes the forward, and an in-place change of a parameter between forward and backward raises as it does in torch).  Positions get no gradient.  Deviations from the reference: a NaN coordinate gives density 0 and no
gradient (the reference indexes the table with NaN * 0); the table gradient is field_training's 64-bit fixed-point sum.
Parameter groups: TrainableFeatureField.get_param_groups() does not know these fields; the caller adds
`{"proposal_networks": [p for f in fields for p in f.parameters()]}` as nerfacto.py's get_param_groups does.  There is no CPU compute path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Mapping, Optional

import numpy as np
import torch

from . import _hashgrid_common as common
from . import _lib
from ._hashgrid_common import SCRATCH_SHIFT_OFFSET, SCRATCH_STATE_OFFSET      # noqa: F401  (tests and scripts read them here)
from ._lib import DensityFieldDesc, DensityFieldGrads, check
from .field_query import growth_factor, nerfstudio_levels, split_tcnn_params, tcnn_levels

WIDTH, MAX_HIDDEN, MAX_INPUT, MAX_POINTS = _lib.DENSITY_FIELD_WIDTH, _lib.DENSITY_FIELD_MAX_LAYERS - 1, _lib.DENSITY_FIELD_MAX_INPUT, 1 << 24
HASH_INIT_SCALE = 0.001


def train_bytes(desc, n: int):
    """(saved_bytes, scratch_bytes) of pixie_density_field_train_bytes"""
    return common.train_bytes("pixie_density_field_train_bytes", desc, n)


def _launch_forward(field, positions, want_raw):
    n = int(positions.shape[0])
    density = torch.empty(n, dtype=torch.float32, device=field.device)
    raw = torch.empty(n, dtype=torch.float32, device=field.device) if want_raw else None
    with torch.cuda.device(field.device):
        check(_lib.load().pixie_density_field_forward(C.byref(field.desc()), positions.data_ptr(), n, density.data_ptr(),
                                                      raw.data_ptr() if raw is not None else None, _lib.current_stream_ptr()),
              "pixie_density_field_forward")
    return density, raw


class _DensityFieldFunction(torch.autograd.Function):
    """args: field, positions (n, 3), want_raw, table, then weights and biases (None where absent) -> density (n,), raw (n,) or None"""

    @staticmethod
    def forward(ctx, field, positions, want_raw, table, *layers):
        density, raw = _launch_forward(field, positions, want_raw)
        ctx.field = field
        # the backward recomputes the forward from the parameters' storage: saving them copies nothing and lets torch's version
        # counters refuse a backward after an in-place change (an optimiser step, mul_) in between
        ctx.save_for_backward(positions, table, *[t for t in layers if t is not None])
        if raw is None:
            return density, None
        ctx.mark_non_differentiable(raw)
        return density, raw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_density, _d_raw):
        field = ctx.field
        positions = ctx.saved_tensors[0]                  # reading them checks that no parameter changed since the forward
        n = int(positions.shape[0])
        need = ctx.needs_input_grad                       # (field, positions, want_raw, table, *layers)
        d_density = d_density.to(torch.float32).contiguous()
        g = DensityFieldGrads()
        grads: List[Optional[torch.Tensor]] = [None, None, None, None]
        if need[3]:
            grads[3] = torch.empty_like(field.table)
            g.d_table = grads[3].data_ptr()
        grads += common.bind_layer_grads(g, list(field.weights) + field.bias_list(), need[4:], field.n_hidden + 1)
        desc = field.desc()
        scratch = common.aligned_scratch(train_bytes(desc, n)[1], field.device)
        with torch.cuda.device(field.device):
            check(_lib.load().pixie_density_field_backward(C.byref(desc), positions.data_ptr(), n, d_density.data_ptr(), C.byref(g),
                                                           scratch.data_ptr(), _lib.current_stream_ptr()), "pixie_density_field_backward")
        _DensityFieldFunction.last_header = scratch[:12].clone()     # bits of max |dX|, shift, state of the latest call (tests read it)
        return tuple(grads)


def _is_linf_contraction(spatial_distortion) -> bool:
    if spatial_distortion is None or spatial_distortion is False:
        return False
    if spatial_distortion is True or spatial_distortion in ("linf", "contraction"):
        return True
    order = getattr(spatial_distortion, "order", None)
    if order is not None and float(order) == float("inf"):
        return True
    raise ValueError("HashMLPDensityField: spatial_distortion must be None (the aabb), True, or a SceneContraction of order inf")


class HashMLPDensityField(torch.nn.Module):
    """The reference's constructor arguments.  num_layers counts the output layer, as nerfstudio's MLP does: num_layers = 2 is one
    hidden layer.  hidden_dim must be 16 (and defaults to it; the reference's default of 64 is TrainableHashMLP's width).
    spatial_distortion: None (positions are normalised by the aabb), True or a SceneContraction of order inf.  implementation selects
    the grid convention: "torch" = nerfstudio_levels with biases, "tcnn" = tcnn_levels without.  world_to_nerf: optional (3, 4) / (4, 4)
    affine applied first.  Parameters: table (rows, F), weights, biases (float32, on `device`)."""

    def __init__(self, aabb, num_layers: int = 2, hidden_dim: int = WIDTH, spatial_distortion=None, use_linear: bool = False, num_levels: int = 8,
                 max_res: int = 1024, base_res: int = 16, log2_hashmap_size: int = 18, features_per_level: int = 2,
                 average_init_density: float = 1.0, implementation: str = "tcnn", world_to_nerf=None, device="cuda:0"):
        super().__init__()
        if implementation not in ("torch", "tcnn"):
            raise ValueError(f"HashMLPDensityField: implementation must be 'torch' or 'tcnn', got {implementation!r}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.PixieHipError("HashMLPDensityField runs on a HIP device only (no CPU fallback)")
        n_hidden = 0 if use_linear else int(num_layers) - 1
        if not use_linear and hidden_dim != WIDTH:
            raise ValueError(f"HashMLPDensityField: hidden_dim {hidden_dim} is not {WIDTH}: this is the 16-wide path; 64-wide networks are "
                             "field_training.TrainableHashMLP")
        if not 0 <= n_hidden <= MAX_HIDDEN or (not use_linear and n_hidden < 1):
            raise ValueError(f"HashMLPDensityField: num_layers {num_layers} gives {n_hidden} hidden layers, outside 1..{MAX_HIDDEN} (0: use_linear)")
        if features_per_level not in (2, 4, 8):
            raise ValueError(f"HashMLPDensityField: features_per_level {features_per_level} is not 2, 4 or 8")
        in_dim = int(num_levels) * int(features_per_level)
        if in_dim > MAX_INPUT:
            raise ValueError(f"HashMLPDensityField: {num_levels} levels x {features_per_level} features = {in_dim} input columns, at most {MAX_INPUT}")
        self.device, self.implementation, self.use_linear = dev, implementation, bool(use_linear)
        self.n_hidden, self.in_dim, self.features_per_level = n_hidden, in_dim, int(features_per_level)
        self.config = dict(num_layers=num_layers, hidden_dim=hidden_dim, use_linear=use_linear, num_levels=num_levels, max_res=max_res,
                           base_res=base_res, log2_hashmap_size=log2_hashmap_size, features_per_level=features_per_level)
        if implementation == "torch":
            self.levels, rows = nerfstudio_levels(num_levels, base_res, max_res, log2_hashmap_size)
        else:
            self.levels, rows = tcnn_levels(num_levels, base_res, growth_factor(num_levels, base_res, max_res), log2_hashmap_size)
        self.contraction = _is_linf_contraction(spatial_distortion)
        self.spatial_distortion = spatial_distortion
        box = np.asarray([[-1.0] * 3, [1.0] * 3] if aabb is None else (aabb.detach().cpu().numpy() if torch.is_tensor(aabb) else aabb), np.float32)
        if box.shape != (2, 3):
            raise ValueError(f"HashMLPDensityField: aabb must be (2, 3), got {box.shape}")
        if not self.contraction and not np.all(box[1] > box[0]):
            raise ValueError("HashMLPDensityField: empty aabb and no spatial_distortion")
        self.register_buffer("aabb", torch.from_numpy(box.copy()).to(dev))
        self._aabb_host = box
        self.average_init_density = float(average_init_density)
        affine = None
        if world_to_nerf is not None:
            a = np.asarray(world_to_nerf, np.float64)[:3]
            if a.shape != (3, 4):
                raise ValueError(f"HashMLPDensityField: world_to_nerf must be (3, 4) or (4, 4), got {np.shape(world_to_nerf)}")
            affine = torch.from_numpy(a.astype(np.float32)).contiguous().to(dev)
        self.register_buffer("world_to_nerf", affine)
        # the reference's initialisation: HashEncoding's uniform(-1, 1) * hash_init_scale, nn.Linear's default for the layers
        self.table = torch.nn.Parameter((torch.rand(rows, self.features_per_level, device=dev) * 2 - 1) * HASH_INIT_SCALE)
        dims = [in_dim] + [WIDTH] * n_hidden + [1]
        with_bias = implementation == "torch" or self.use_linear
        weights, biases = [], []
        for i in range(len(dims) - 1):
            bound = 1.0 / math.sqrt(dims[i])
            weights.append(torch.nn.Parameter((torch.rand(dims[i + 1], dims[i], device=dev) * 2 - 1) * bound))
            biases.append(torch.nn.Parameter((torch.rand(dims[i + 1], device=dev) * 2 - 1) * bound) if with_bias else None)
        self.weights = torch.nn.ParameterList(weights)
        self._set_biases(biases)

    def _set_biases(self, biases):
        self.bias_layers = [i for i, b in enumerate(biases) if b is not None]
        self.biases = torch.nn.ParameterList([b for b in biases if b is not None])

    def _load(self, table, weights, biases):
        """replaces the parameters' values (and which layers have a bias) after checking every shape"""
        dev = self.device
        as_t = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32))).detach().to(
            device=dev, dtype=torch.float32).contiguous().clone()
        table = as_t(table)
        if tuple(table.shape) != tuple(self.table.shape):
            raise ValueError(f"HashMLPDensityField: the hash table is {tuple(table.shape)}, the configuration implies {tuple(self.table.shape)}")
        if len(weights) != self.n_hidden + 1 or len(biases) != self.n_hidden + 1:
            raise ValueError(f"HashMLPDensityField: {len(weights)} layers given, the configuration implies {self.n_hidden + 1}")
        new_w, new_b = [], []
        for i, (w, b) in enumerate(zip(weights, biases)):
            w = as_t(w)
            if tuple(w.shape) != tuple(self.weights[i].shape):
                raise ValueError(f"HashMLPDensityField: layer {i} is {tuple(w.shape)}, expected {tuple(self.weights[i].shape)}")
            if b is not None:
                b = as_t(b)
                if tuple(b.shape) != (w.shape[0],):
                    raise ValueError(f"HashMLPDensityField: bias {i} is {tuple(b.shape)}, expected {(w.shape[0],)}")
            new_w.append(torch.nn.Parameter(w))
            new_b.append(torch.nn.Parameter(b) if b is not None else None)
        self.table = torch.nn.Parameter(table)
        self.weights = torch.nn.ParameterList(new_w)
        self._set_biases(new_b)
        return self

    # ---- constructors ----
    @classmethod
    def from_arrays(cls, table, weights, biases=None, **config) -> "HashMLPDensityField":
        """explicit arrays for a field of the given constructor arguments"""
        self = cls(**config)
        return self._load(table, list(weights), [None] * len(weights) if biases is None else list(biases))

    @classmethod
    def from_nerfstudio_state_dict(cls, state_dict: Mapping, prefix: str, config: Mapping) -> "HashMLPDensityField":
        """The torch-implementation keys of the reference module: {prefix}.mlp_base.0.hash_table and {prefix}.mlp_base.1.layers.K.weight|bias;
        with use_linear the table ({prefix}.encoding.hash_table, or the key above) and {prefix}.linear.weight|bias.
        config: the constructor's arguments (implementation defaults to "torch" here)."""
        config = dict(config)
        config.setdefault("implementation", "torch")
        self = cls(**config)
        sd = state_dict
        if self.use_linear:
            key = f"{prefix}.encoding.hash_table" if f"{prefix}.encoding.hash_table" in sd else f"{prefix}.mlp_base.0.hash_table"
            return self._load(sd[key], [sd[f"{prefix}.linear.weight"]], [sd.get(f"{prefix}.linear.bias")])
        ws, bs, k = [], [], 0
        while f"{prefix}.mlp_base.1.layers.{k}.weight" in sd:
            ws.append(sd[f"{prefix}.mlp_base.1.layers.{k}.weight"])
            bs.append(sd.get(f"{prefix}.mlp_base.1.layers.{k}.bias"))
            k += 1
        if not ws:
            raise KeyError(f"from_nerfstudio_state_dict: no '{prefix}.mlp_base.1.layers.0.weight' in the state dict")
        return self._load(sd[f"{prefix}.mlp_base.0.hash_table"], ws, bs)

    @classmethod
    def from_tcnn_params(cls, encoding_params, network_params, config: Mapping) -> "HashMLPDensityField":
        """The two flat tiny-cuda-nn vectors of the reference module: the grid's (rows x F, level after level) and the FullyFusedMLP's,
        in split_tcnn_params' layout for a 16-wide network.  Refuses unless both counts are exact.  use_linear has no tiny-cuda-nn
        form (the reference's linear layer is a torch module): use from_nerfstudio_state_dict."""
        config = dict(config)
        config.setdefault("implementation", "tcnn")
        self = cls(**config)
        if self.use_linear:
            raise ValueError("from_tcnn_params: use_linear is a torch.nn.Linear in the reference; use from_nerfstudio_state_dict")
        enc = encoding_params.detach().cpu().numpy() if torch.is_tensor(encoding_params) else np.asarray(encoding_params)
        enc = enc.reshape(-1).astype(np.float32)
        rows, F = self.table.shape
        if enc.size != rows * F:
            raise ValueError(f"from_tcnn_params: the grid implies {rows} x {F} = {rows * F} parameters, encoding_params holds {enc.size}")
        ws, bs, _ = split_tcnn_params(network_params, self.in_dim, self.n_hidden, 1, width=WIDTH)
        return self._load(enc.reshape(rows, F), ws, bs)

    # ---- the descriptor ----
    def bias_list(self):
        return common.bias_list(self.bias_layers, self.biases, self.n_hidden + 1)

    def desc(self) -> DensityFieldDesc:
        """over the parameters' own storage: it follows optimiser steps, nothing is copied"""
        common.require_device_params(self, self.device, "HashMLPDensityField")
        d = DensityFieldDesc()
        d.n_levels, d.features_per_level, d.n_hidden, d.hidden_width = len(self.levels), self.features_per_level, self.n_hidden, WIDTH
        d.contraction, d.average_init_density = int(self.contraction), self.average_init_density
        common.fill_levels(d, self.levels)
        d.d_table, d.table_rows = self.table.data_ptr(), int(self.table.shape[0])
        for i, (w, b) in enumerate(zip(self.weights, self.bias_list())):
            d.d_weight[i] = w.data_ptr()
            d.d_bias[i] = b.data_ptr() if b is not None else None
        d.d_world_to_nerf = self.world_to_nerf.data_ptr() if self.world_to_nerf is not None else None
        d.aabb = (C.c_float * 6)(*self._aabb_host.reshape(-1).tolist())
        return d

    # ---- the reference's surface ----
    def forward(self, positions, return_raw: bool = False):
        """positions (..., 3) in the nerf frame (the world frame with world_to_nerf) -> densities (..., 1); with return_raw also the
        pre-activation h (..., 1), which carries no gradient"""
        if not torch.is_tensor(positions) or positions.device != self.device:
            raise _lib.PixieHipError(f"HashMLPDensityField: positions must be a tensor on {self.device} (no CPU fallback)")
        if positions.requires_grad:
            raise ValueError("HashMLPDensityField: positions get no gradient (the reference needs one for predict_normals only, which is "
                             "off by default); detach them")
        if positions.shape[-1] != 3:
            raise ValueError(f"HashMLPDensityField: positions must be (..., 3), got {tuple(positions.shape)}")
        lead = tuple(positions.shape[:-1])
        flat = positions.reshape(-1, 3).to(torch.float32).contiguous()
        n = int(flat.shape[0])
        if n > MAX_POINTS:
            raise ValueError(f"HashMLPDensityField: {n} points in one call, at most 2^24")
        self.desc()                                        # the parameter checks, before autograd sees the call
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            density, raw = _DensityFieldFunction.apply(self, flat, bool(return_raw), self.table, *self.weights, *self.bias_list())
        else:
            density, raw = _launch_forward(self, flat, bool(return_raw))
        density = density.reshape(*lead, 1)
        return (density, raw.reshape(*lead, 1)) if return_raw else density

    def density_fn(self, positions):
        """what ProposalNetworkSampler calls: positions (R, S, 3) -> densities (R, S, 1)"""
        return self.forward(positions)

    def get_density(self, ray_samples):
        return self.forward(ray_samples.frustums.get_positions()), None

    # ---- the 64-wide twin ----
    def to_trainable_hashmlp(self):
        """A field_training.TrainableHashMLP with this network zero-padded to 64 hidden units (copies): positions in the unit cube,
        times the selector, -> h.  Contraction, selector and trunc_exp stay with the caller, as torch ops.  use_linear has no twin."""
        from .field_training import TrainableHashMLP
        if self.n_hidden < 1:
            raise ValueError("HashMLPDensityField: use_linear has no 64-wide twin (HashMLP needs a hidden layer)")
        dev, biases = self.device, self.bias_list()
        ws, bs = [], []
        for i, w in enumerate(self.weights):
            out_pad = 64 if i < self.n_hidden else 1
            in_pad = self.in_dim if i == 0 else 64
            wp = torch.zeros(out_pad, in_pad, device=dev)
            wp[:w.shape[0], :w.shape[1]] = w.detach()
            ws.append(wp)
            if biases[i] is None:
                bs.append(None)
            else:
                bp = torch.zeros(out_pad, device=dev)
                bp[:w.shape[0]] = biases[i].detach()
                bs.append(bp)
        return TrainableHashMLP(self.levels, self.table.detach().clone(), ws, bs, device=dev)
