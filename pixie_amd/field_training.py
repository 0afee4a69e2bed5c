"""Differentiable hash-grid MLPs: the trainable counterpart of field_query.HashMLP, with tiny-cuda-nn's role in the F3RM model.

The reference trains its field with `ns-train f3rm` (pipeline.py:84-132); all three networks of that model are
tcnn.NetworkWithInputEncoding / FullyFusedMLP modules (nerfacto_field.py, f3rm/feature_field.py:71-82), which exist for CUDA only.
What they give FeatureFieldModel.get_outputs / get_loss_dict is a module that maps positions to outputs with gradients for the hash
table and the MLP weights under torch.autograd.  This file is that module over pixie_amd/csrc/field_query_backward.hip; everything above it
(ray sampling, the losses, torch.optim.Adam) is plain torch, except get_weights and the renderers: pixie_amd/ray_render.py.

    TrainableHashMLP(levels, table, weights, biases, ...)    torch.nn.Module; parameters table, weights, biases; forward(positions, extra)
    TrainableHashMLP.from_hashmlp(h) / .to_hashmlp()         both ways over the same storage
    TrainableFeatureField(density, color, feature, ...)      the three networks; get_param_groups(); to_query() -> FeatureFieldQuery

Differentiable: the parameters and `extra` (how the colour head's loss reaches the density net's geometry features).  Not
differentiable: positions (the reference detaches them for the feature net and needs them for normals only, predict_normals,
off by default), and the backward itself (no double backward).  Deviations from torch's own autograd on the same expression
(INTEGRATION 1a): the table gradient is a 64-bit fixed-point sum, bit-identical from run to run and under a permutation of the
points, each contribution off by at most 2^(-s-1) with s in the scratch header; an Inf or NaN anywhere in the grid columns' gradient
makes the WHOLE table gradient NaN (torch: the touched rows only).  There is no CPU compute path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import torch

from . import _hashgrid_common as common
from . import _lib
from ._hashgrid_common import SCRATCH_SHIFT_OFFSET, SCRATCH_STATE_OFFSET      # noqa: F401  (tests and scripts read them here)
from ._lib import HashMlpGrads, check
from .field_query import ACTIVATIONS, FeatureFieldQuery, HashMLP


def train_bytes(desc, n: int):
    """(saved_bytes, scratch_bytes) of pixie_hashmlp_train_bytes"""
    return common.train_bytes("pixie_hashmlp_train_bytes", desc, n)


class _HashMlpFunction(torch.autograd.Function):
    """args: net (HashMLP over the parameters' storage), positions, extra, table, then weights and biases (None where absent)"""

    @staticmethod
    def forward(ctx, net: HashMLP, positions, extra, table, *layers):
        n = int((positions if positions is not None else extra).shape[0])
        dev = net.device
        out = torch.empty((n, net.out_dim), dtype=torch.float32, device=dev)
        desc = net.desc()
        saved_bytes, scratch_bytes = train_bytes(desc, n)
        saved = torch.empty(max(saved_bytes, 4) // 4, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(_lib.load().pixie_hashmlp_forward_saved(C.byref(desc), positions.data_ptr() if positions is not None else None,
                                                          extra.data_ptr() if extra is not None else None, n, out.data_ptr(), saved.data_ptr(),
                                                          _lib.current_stream_ptr()), "pixie_hashmlp_forward_saved")
        ctx.net, ctx.n, ctx.scratch_bytes = net, n, scratch_bytes
        ctx.has = (positions is not None, extra is not None, table is not None, [t is not None for t in layers])
        ctx.save_for_backward(*[t for t in (positions, extra, table, *layers) if t is not None], out, saved)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out):
        net, n = ctx.net, ctx.n
        tensors = list(ctx.saved_tensors)
        saved, out = tensors.pop(), tensors.pop()
        has_pos, has_extra, has_table, has_layers = ctx.has
        positions = tensors.pop(0) if has_pos else None
        extra = tensors.pop(0) if has_extra else None
        table = tensors.pop(0) if has_table else None
        need = ctx.needs_input_grad                       # (net, positions, extra, table, *layers)
        dev = net.device
        d_out = d_out.to(torch.float32).contiguous()
        g = HashMlpGrads()
        grads: List[Optional[torch.Tensor]] = [None, None, None, None]
        if has_extra and need[2]:
            grads[2] = torch.empty_like(extra)
            g.d_extra = grads[2].data_ptr()
        if has_table and need[3]:
            grads[3] = torch.empty_like(table)
            g.d_table = grads[3].data_ptr()
        layers = [tensors.pop(0) if present else None for present in has_layers]
        grads += common.bind_layer_grads(g, layers, need[4:], net.n_hidden + 1)
        scratch = common.aligned_scratch(ctx.scratch_bytes, dev)
        with torch.cuda.device(dev):
            check(_lib.load().pixie_hashmlp_backward(C.byref(net.desc()), positions.data_ptr() if positions is not None else None,
                                                     extra.data_ptr() if extra is not None else None, n, out.data_ptr(), saved.data_ptr(),
                                                     d_out.data_ptr(), C.byref(g), scratch.data_ptr(), _lib.current_stream_ptr()),
                  "pixie_hashmlp_backward")
        _HashMlpFunction.last_header = scratch[:12].clone()     # bits of max |dX_grid|, shift, state of the latest call (tests read it)
        return tuple(grads)


class TrainableHashMLP(torch.nn.Module):
    """field_query.HashMLP's constructor arguments; `table`, `weights` (ParameterList) and `biases` (ParameterList, empty slots for
    layers without a bias) are the parameters, float32 on the device.  forward(positions, extra=None) -> (n, out_dim), through one
    autograd.Function; under torch.no_grad(), or when nothing requires a gradient, it is HashMLP.__call__ and saves nothing."""

    def __init__(self, levels, table, weights, biases=None, n_frequencies: int = 0, n_extra: int = 0, out_activation="none", device="cuda:0"):
        super().__init__()
        self._adopt(HashMLP(levels, table, weights, biases, n_frequencies, n_extra, out_activation, device), out_activation)

    def _adopt(self, h: HashMLP, out_activation):
        self.levels, self.n_frequencies, self.n_extra, self.out_activation = h.levels, h.n_frequencies, h.n_extra, out_activation
        self.in_dim, self.out_dim, self.n_hidden, self.device = h.in_dim, h.out_dim, h.n_hidden, h.device
        self.table = torch.nn.Parameter(h.table) if h.table is not None else None
        self.weights = torch.nn.ParameterList([torch.nn.Parameter(w) for w in h.weights])
        self.bias_layers = [i for i, b in enumerate(h.biases) if b is not None]
        self.biases = torch.nn.ParameterList([torch.nn.Parameter(b) for b in h.biases if b is not None])

    @classmethod
    def from_hashmlp(cls, h: HashMLP) -> "TrainableHashMLP":
        """the parameters are h's own tensors: nothing is copied"""
        self = cls.__new__(cls)
        torch.nn.Module.__init__(self)
        self._adopt(h, {v: k for k, v in ACTIVATIONS.items() if k is not None}[h.out_activation])
        return self

    def bias_list(self):
        return common.bias_list(self.bias_layers, self.biases, self.n_hidden + 1)

    def to_hashmlp(self) -> HashMLP:
        """a HashMLP over the parameters' storage (it follows optimiser steps; nothing is copied)"""
        common.require_device_params(self, self.device, "TrainableHashMLP")
        return HashMLP(self.levels if len(self.levels) else None, self.table, list(self.weights), self.bias_list(), self.n_frequencies, self.n_extra,
                       self.out_activation, self.device)

    def forward(self, positions=None, extra=None) -> torch.Tensor:
        net = self.to_hashmlp()
        if positions is not None and torch.is_tensor(positions) and positions.requires_grad:
            raise ValueError("TrainableHashMLP: positions get no gradient (the reference needs one for predict_normals only, which is "
                             "off by default); detach them")
        wants = torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or (torch.is_tensor(extra) and extra.requires_grad))
        if not wants:
            return net(positions, extra)
        _, positions, extra = net.check_inputs(positions, extra, "TrainableHashMLP", 1 << 24)
        return _HashMlpFunction.apply(net, positions, extra, self.table, *self.weights, *self.bias_list())


class TrainableFeatureField(torch.nn.Module):
    """The density net, the colour head and the feature net of a feature field as TrainableHashMLPs.  Built from a FeatureFieldQuery
    (from_query) or by its constructors (from_arrays, from_nerfstudio_state_dict, from_tcnn_params: same arguments); to_query() returns
    a FeatureFieldQuery over the same storage, for voxelize()."""

    def __init__(self, density: TrainableHashMLP, color: TrainableHashMLP, feature: TrainableHashMLP, world_to_nerf=None, contraction: bool = True,
                 aabb=None, average_init_density: float = 1.0):
        super().__init__()
        self.density, self.color, self.feature = density, color, feature
        self.query_args = dict(world_to_nerf=world_to_nerf, contraction=contraction, aabb=aabb, average_init_density=average_init_density)
        self.to_query()                                    # FeatureFieldQuery's checks of the three shapes

    @classmethod
    def from_query(cls, q: FeatureFieldQuery) -> "TrainableFeatureField":
        return cls(TrainableHashMLP.from_hashmlp(q.density), TrainableHashMLP.from_hashmlp(q.color), TrainableHashMLP.from_hashmlp(q.feature),
                   q.world_to_nerf, q.contraction, q.aabb, q.average_init_density)

    @classmethod
    def from_arrays(cls, *args, **kwargs) -> "TrainableFeatureField":
        return cls.from_query(FeatureFieldQuery.from_arrays(*args, **kwargs))

    @classmethod
    def from_nerfstudio_state_dict(cls, *args, **kwargs) -> "TrainableFeatureField":
        return cls.from_query(FeatureFieldQuery.from_nerfstudio_state_dict(*args, **kwargs))

    @classmethod
    def from_tcnn_params(cls, *args, **kwargs) -> "TrainableFeatureField":
        return cls.from_query(FeatureFieldQuery.from_tcnn_params(*args, **kwargs))

    def get_param_groups(self) -> Dict[str, List[torch.nn.Parameter]]:
        """the reference's grouping (f3rm/model.py get_param_groups over nerfacto's): "fields" = the nerfacto field (density net and
        colour head), "feature_field" = the feature net"""
        return {"fields": list(self.density.parameters()) + list(self.color.parameters()), "feature_field": list(self.feature.parameters())}

    def to_query(self) -> FeatureFieldQuery:
        return FeatureFieldQuery(self.density.to_hashmlp(), self.color.to_hashmlp(), self.feature.to_hashmlp(), **self.query_args)

    def forward(self, positions):
        """unit-cube positions (n, 3) -> dict(density_out (n, 1 + G), rgb (n, 3), feature (n, C)): the density net's raw outputs, the
        colour head on its geometry columns, the feature net"""
        h = self.density(positions)
        return {"density_out": h, "rgb": self.color(None, h[:, 1:]), "feature": self.feature(positions)}
