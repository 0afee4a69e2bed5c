"""NeRF feature-field query on the device: hash grids, fused MLPs and the voxeliser.

Mirrors pixie/voxel/voxelize.py: `extract_clip_voxel_grid` (:17-141), the stage that turns a trained F3RM model into the
`*_features.npy`, `*_alphas.npy`, `*_rgb.npy` and `*_mask.npy` files everything downstream reads.  The reference queries
f3rm_robot/field_adapter.py's FeatureFieldAdapter 4096 points at a time; the three networks underneath (the nerfacto density net
and colour head, nerfacto_field.py:134-146, 193-232, 297-308, and the feature net, f3rm/feature_field.py:47-113) run on
tiny-cuda-nn, which is CUDA-only.  Here one pixie_field_voxelize call (HIP, pixie_amd/csrc/field_query.hip) walks the whole lattice in
two launches on torch's current stream, without a stream synchronise or a host read-back.

    HashMLP(levels, table, weights, biases, ...)            one grid -> MLP network; __call__(positions, extra) -> (n, out) float32
    nerfstudio_levels(...) / tcnn_levels(...)               the two grid conventions as level tables
    FeatureFieldQuery.from_arrays / from_nerfstudio_state_dict / from_tcnn_params
    FeatureFieldQuery.__call__ / get_density / get_alpha / get_rgb      FeatureFieldAdapter's surface (float32, any point set)
    FeatureFieldQuery.voxelize(min_bounds, max_bounds, voxel_size)       the fused lattice call (float16 grids)
    extract_clip_voxel_grid(field, output_path, bounds, voxel_size)      writes the reference's files
    voxelize_to_device(field, bounds, voxel_size)                        (feat_grid, mask, min_bounds, max_bounds) for neural_scene_rollout

Two grid conventions share the kernel through a per-level table {scale, shift, res, size, offset, dense} (include/pixie_hip.h):
"nerfstudio" is nerfstudio's torch HashEncoding (field_components/encodings.py:343-347, 401-460), "tcnn" the published
tiny-cuda-nn grid.  The colour head's direction input is constant for this query (the adapter passes zero directions) and so is the
eval-time appearance embedding; both are folded into the first layer's bias on the host, which leaves a G -> 64 -> ... -> 3 head.
nerfstudio's eval_setup is not restated: the caller supplies arrays or a state dict.  There is no CPU compute path.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._hashgrid_common import fill_levels
from ._lib import FieldVoxelizeDesc, HashMlpDesc, check

MAX_LEVELS, MAX_HIDDEN, MAX_INPUT, MAX_OUTPUT, WIDTH = _lib.HASHMLP_MAX_LEVELS, _lib.HASHMLP_MAX_LAYERS - 1, _lib.HASHMLP_MAX_INPUT, _lib.HASHMLP_MAX_OUTPUT, 64
ACTIVATIONS = {"none": 0, None: 0, "sigmoid": 1, "exp": 2}
LEVEL_DTYPE = np.dtype([("scale", "f4"), ("shift", "f4"), ("res", "u4"), ("size", "u4"), ("offset", "u4"), ("dense", "u4")])


# ------------------------------------------------------------------------------------------------------------------------------
# level tables
# ------------------------------------------------------------------------------------------------------------------------------
def growth_factor(num_levels: int, min_res: int, max_res: int) -> float:
    """exp((ln max_res - ln min_res) / (L - 1)), in double (encodings.py:344, feature_field.py:47)"""
    return float(np.exp((np.log(max_res) - np.log(min_res)) / (num_levels - 1))) if num_levels > 1 else 1.0


def nerfstudio_levels(num_levels: int, min_res: int, max_res: int, log2_hashmap_size: int):
    """HashEncoding's torch path: scale = floor(min_res * growth^l), always hashed, 2^T rows per level.  The power is taken in
    float32, as torch evaluates `growth ** torch.arange(L)` (a double raised to an integer tensor gives the default dtype): 16
    levels from 16 to 2048 end at 2047.  Returns (levels, total rows)."""
    _check_levels(num_levels, log2_hashmap_size)
    g = np.float32(growth_factor(num_levels, min_res, max_res))
    lv = np.zeros(num_levels, LEVEL_DTYPE)
    lv["scale"] = np.floor(np.float32(min_res) * np.power(g, np.arange(num_levels, dtype=np.float32)))
    lv["res"] = lv["scale"].astype(np.uint32) + 1
    lv["size"] = 1 << log2_hashmap_size
    lv["offset"] = np.arange(num_levels, dtype=np.uint32) << log2_hashmap_size
    return lv, num_levels << log2_hashmap_size


def tcnn_levels(num_levels: int, base_res: int, per_level_scale: float, log2_hashmap_size: int):
    """tiny-cuda-nn's HashGrid: scale = exp2(l log2 s) base - 1 (in double, rounded once to float32), shift 0.5, res = ceil(scale) + 1, dense while res^3 <=
    2^T, a level holds min(roundup8(res^3), 2^T) rows and the levels are packed one after another.  Returns (levels, total rows)."""
    _check_levels(num_levels, log2_hashmap_size)
    T = 1 << log2_hashmap_size
    log2s = math.log2(per_level_scale)
    lv = np.zeros(num_levels, LEVEL_DTYPE)
    offset = 0
    for l in range(num_levels):
        scale = np.float32(2.0 ** (l * log2s) * base_res - 1.0)
        res = int(np.ceil(scale)) + 1
        size = min((res ** 3 + 7) // 8 * 8, T)
        lv[l] = (scale, 0.5, res, size, offset, 1 if res ** 3 <= T else 0)
        offset += size
    return lv, offset


def _check_levels(num_levels, log2_T):
    if not 1 <= num_levels <= MAX_LEVELS:
        raise ValueError(f"field_query: {num_levels} levels outside 1..{MAX_LEVELS}")
    if not 1 <= log2_T <= 24:
        raise ValueError(f"field_query: log2_hashmap_size {log2_T} outside 1..24")


def sh_components(levels: int, direction: Sequence[float]) -> np.ndarray:
    """Real spherical harmonics of degree < levels <= 4 at one direction, float64, in nerfstudio's component order
    (utils/math.py:29).  The constants are the closed forms sqrt((2l + 1) / (4 pi) ...) evaluated here."""
    if not 1 <= levels <= 4:
        raise ValueError(f"sh_components: levels {levels} outside 1..4")
    x, y, z = (float(v) for v in direction)
    xx, yy, zz, pi, s = x * x, y * y, z * z, math.pi, math.sqrt
    out = [0.5 * s(1 / pi)]
    if levels > 1:
        c = s(3 / (4 * pi))
        out += [c * y, c * z, c * x]
    if levels > 2:
        c = 0.5 * s(15 / pi)
        out += [c * x * y, c * y * z, 0.25 * s(5 / pi) * (3 * zz - 1), c * x * z, 0.25 * s(15 / pi) * (xx - yy)]
    if levels > 3:
        out += [0.25 * s(35 / (2 * pi)) * y * (3 * xx - yy), 0.5 * s(105 / pi) * x * y * z, 0.25 * s(21 / (2 * pi)) * y * (5 * zz - 1),
                0.25 * s(7 / pi) * z * (5 * zz - 3), 0.25 * s(21 / (2 * pi)) * x * (5 * zz - 1), 0.25 * s(105 / pi) * z * (xx - yy),
                0.25 * s(35 / (2 * pi)) * x * (xx - 3 * yy)]
    return np.asarray(out, np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# one network
# ------------------------------------------------------------------------------------------------------------------------------
def _device_f32(a, dev, what):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.float32))
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


class HashMLP:
    """One "hash-grid encoding -> MLP" network resident on the device.

    levels       structured array of LEVEL_DTYPE (nerfstudio_levels / tcnn_levels), or None for a network without a grid
    table        (rows, F) float array, F in {2, 4, 8}; rows must cover every level's offset + size
    weights      n_hidden + 1 matrices (out, in) row-major: hidden layers 64 wide, 1..4 of them, then the output layer (<= 1024)
    biases       None, or one vector / None per layer
    n_frequencies  0, or the octaves of the frequency block appended after the grid columns (tiny-cuda-nn's ordering)
    n_extra      float32 input columns appended last, given to __call__ as `extra`
    out_activation "none", "sigmoid" or "exp"
    Anything outside these limits raises, here or through pixie_last_error()."""

    def __init__(self, levels, table, weights, biases=None, n_frequencies: int = 0, n_extra: int = 0, out_activation="none", device="cuda:0"):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.PixieHipError("HashMLP runs on a HIP device only (no CPU fallback)")
        if out_activation not in ACTIVATIONS:
            raise ValueError(f"HashMLP: out_activation must be one of 'none', 'sigmoid', 'exp', got {out_activation!r}")
        self.device = dev
        self.levels = np.zeros(0, LEVEL_DTYPE) if levels is None else np.ascontiguousarray(levels, dtype=LEVEL_DTYPE)
        if len(self.levels) > MAX_LEVELS:
            raise ValueError(f"HashMLP: {len(self.levels)} levels, at most {MAX_LEVELS}")
        self.table = None
        self.features_per_level = 0
        if len(self.levels):
            self.table = _device_f32(table, dev, "table")
            if self.table.dim() != 2 or self.table.shape[1] not in (2, 4, 8):
                raise ValueError(f"HashMLP: table must be (rows, F) with F in 2, 4, 8, got {tuple(self.table.shape)}")
            self.features_per_level = int(self.table.shape[1])
            need = int((self.levels["offset"].astype(np.int64) + self.levels["size"].astype(np.int64)).max())
            if need > self.table.shape[0] or int(self.levels["size"].min()) < 1:
                raise ValueError(f"HashMLP: the levels need {need} table rows, the table has {self.table.shape[0]}")
        self.n_frequencies, self.n_extra = int(n_frequencies), int(n_extra)
        self.in_dim = len(self.levels) * self.features_per_level + 6 * self.n_frequencies + self.n_extra
        if not 1 <= self.in_dim <= MAX_INPUT:
            raise ValueError(f"HashMLP: input row of {self.in_dim} columns outside 1..{MAX_INPUT}")
        weights = list(weights)
        if not 2 <= len(weights) <= MAX_HIDDEN + 1:
            raise ValueError(f"HashMLP: {len(weights) - 1} hidden layers outside 1..{MAX_HIDDEN}")
        biases = [None] * len(weights) if biases is None else list(biases)
        if len(biases) != len(weights):
            raise ValueError("HashMLP: one bias (or None) per layer")
        self.weights, self.biases = [], []
        fan_in = self.in_dim
        for i, (w, b) in enumerate(zip(weights, biases)):
            w = _device_f32(w, dev, "weight")
            last = i == len(weights) - 1
            if w.dim() != 2 or w.shape[1] != fan_in or (not last and w.shape[0] != WIDTH):
                raise ValueError(f"HashMLP: layer {i} must be ({'out' if last else WIDTH}, {fan_in}), got {tuple(w.shape)}: hidden layers are {WIDTH} wide")
            if b is not None:
                b = _device_f32(b, dev, "bias")
                if tuple(b.shape) != (w.shape[0],):
                    raise ValueError(f"HashMLP: bias {i} must be ({w.shape[0]},), got {tuple(b.shape)}")
            self.weights.append(w)
            self.biases.append(b)
            fan_in = WIDTH
        self.n_hidden, self.out_dim = len(weights) - 1, int(self.weights[-1].shape[0])
        if not 1 <= self.out_dim <= MAX_OUTPUT:
            raise ValueError(f"HashMLP: out_dim {self.out_dim} outside 1..{MAX_OUTPUT}")
        self.out_activation = ACTIVATIONS[out_activation]

    def fill(self, d: HashMlpDesc) -> HashMlpDesc:
        d.n_levels, d.features_per_level = len(self.levels), self.features_per_level
        d.n_frequencies, d.n_extra, d.n_hidden, d.out_dim, d.out_activation = self.n_frequencies, self.n_extra, self.n_hidden, self.out_dim, self.out_activation
        fill_levels(d, self.levels)
        d.d_table = self.table.data_ptr() if self.table is not None else None
        d.table_rows = int(self.table.shape[0]) if self.table is not None else 0
        for i, (w, b) in enumerate(zip(self.weights, self.biases)):
            d.d_weight[i] = w.data_ptr()
            d.d_bias[i] = b.data_ptr() if b is not None else None
        return d

    def desc(self) -> HashMlpDesc:
        return self.fill(HashMlpDesc())

    def check_inputs(self, positions, extra, who="HashMLP", max_points=None):
        """the checks of a call's inputs, under the name `who` (TrainableHashMLP shares them) -> (n, positions, extra), both
        contiguous float32"""
        given = [t for t in (positions, extra) if t is not None]
        if not given:
            raise ValueError(f"{who}: no input")
        for t in given:
            if not torch.is_tensor(t) or t.device != self.device:
                raise _lib.PixieHipError(f"{who}: inputs must be tensors on {self.device} (no CPU fallback)")
        n = int(given[0].shape[0])
        if max_points is not None and n > max_points:
            raise ValueError(f"{who}: {n} points in one call, at most 2^24")
        if positions is not None:
            if positions.dim() != 2 or positions.shape[1] != 3:
                raise ValueError(f"{who}: positions must be (n, 3), got {tuple(positions.shape)}")
            positions = positions.to(torch.float32).contiguous()
        elif len(self.levels) or self.n_frequencies:
            raise ValueError(f"{who}: this network needs positions")
        if (extra is not None) != (self.n_extra > 0):
            raise ValueError(f"{who}: extra must be given iff n_extra > 0 (n_extra = {self.n_extra})")
        if extra is not None:
            if tuple(extra.shape) != (n, self.n_extra):
                raise ValueError(f"{who}: extra must be {(n, self.n_extra)}, got {tuple(extra.shape)}")
            extra = extra.to(torch.float32).contiguous()
        return n, positions, extra

    def __call__(self, positions=None, extra=None) -> torch.Tensor:
        """positions (n, 3) float32 unit-cube device tensor (None for a network without grid and frequency block), extra
        (n, n_extra) -> (n, out_dim) float32.  One launch on the current stream."""
        n, positions, extra = self.check_inputs(positions, extra)
        out = torch.empty((n, self.out_dim), dtype=torch.float32, device=self.device)
        lib = _lib.load()
        with torch.cuda.device(self.device):
            check(lib.pixie_hashmlp_forward(C.byref(self.desc()), positions.data_ptr() if positions is not None else None,
                                            extra.data_ptr() if extra is not None else None, n, out.data_ptr(), _lib.current_stream_ptr()),
                  "pixie_hashmlp_forward")
        return out


# ------------------------------------------------------------------------------------------------------------------------------
# the three networks of a feature field
# ------------------------------------------------------------------------------------------------------------------------------
def fold_color_head(weights, biases, n_direction: int, n_geo: int, direction_encoding, appearance=None):
    """The colour head (nerfacto_field.py:297-307) takes [direction encoding | geometry | appearance].  With the first and the last
    constant, W0 h + b0 = W0[:, geo] geo + (b0 + W0[:, dir] d + W0[:, app] a): returns (weights, biases) of the G-input head, the
    fold done in float64."""
    w0 = np.asarray(weights[0], np.float64)
    n_app = 0 if appearance is None else len(appearance)
    if w0.shape[1] != n_direction + n_geo + n_app:
        raise ValueError(f"fold_color_head: first layer has {w0.shape[1]} inputs, expected {n_direction} + {n_geo} + {n_app}")
    b0 = np.zeros(w0.shape[0]) if biases is None or biases[0] is None else np.asarray(biases[0], np.float64)
    b0 = b0 + w0[:, :n_direction] @ np.asarray(direction_encoding, np.float64)
    if n_app:
        b0 = b0 + w0[:, n_direction + n_geo:] @ np.asarray(appearance, np.float64)
    rest = [None] * (len(weights) - 1) if biases is None else list(biases[1:])
    return [w0[:, n_direction:n_direction + n_geo].astype(np.float32)] + list(weights[1:]), [b0.astype(np.float32)] + rest


def split_tcnn_params(params, in_dim: int, n_hidden: int, out_dim: int, table_rows: int = 0, features_per_level: int = 0, pad_value: float = 1.0,
                      width: int = WIDTH):
    """The flat `params` vector of a tiny-cuda-nn FullyFusedMLP (+ grid) in the published layout: network weights first, then the
    grid; each layer (out, in) row-major without bias; the first layer's `in` and the last layer's `out` padded to multiples of 16;
    the padding input columns hold `pad_value` (1.0), so their weights sum into a bias.  `width`: the hidden layers' width (64; 16 for
    the proposal density fields).  Refuses unless the count this implies
    equals params.numel() exactly.  Returns (weights, biases, table or None)."""
    p = params.detach().cpu().numpy() if torch.is_tensor(params) else np.asarray(params)
    p = p.reshape(-1).astype(np.float32)
    in_pad, out_pad = (in_dim + 15) // 16 * 16, (out_dim + 15) // 16 * 16
    shapes = [(width, in_pad)] + [(width, width)] * (n_hidden - 1) + [(out_pad, width)]
    expect = sum(a * b for a, b in shapes) + table_rows * features_per_level
    if p.size != expect:
        raise ValueError(f"split_tcnn_params: the layout implies {expect} parameters ({shapes} + {table_rows} x {features_per_level} grid), "
                         f"params holds {p.size}")
    mats, at = [], 0
    for a, b in shapes:
        mats.append(p[at:at + a * b].reshape(a, b))
        at += a * b
    table = p[at:].reshape(table_rows, features_per_level) if table_rows else None
    biases = [None] * len(mats)
    if in_pad > in_dim:
        biases[0] = (mats[0][:, in_dim:].astype(np.float64).sum(axis=1) * pad_value).astype(np.float32)
        mats[0] = np.ascontiguousarray(mats[0][:, :in_dim])
    mats[-1] = np.ascontiguousarray(mats[-1][:out_dim])
    return mats, biases, table


class FeatureFieldQuery:
    """FeatureFieldAdapter's surface (field_adapter.py:28-72) over three HashMLPs, plus the fused lattice call.

    density   positions -> 1 + G columns: log density and the geometry features (no activation)
    color     G geometry columns -> 3, sigmoid: the folded colour head
    feature   positions -> C columns
    world_to_nerf  (3, 4) or (4, 4) affine applied as n_r = ((A[r][0] x + A[r][1] y) + A[r][2] z) + A[r][3]; None = identity
    contraction    True: L-infinity scene contraction then (p + 2) / 4; False: (p - aabb[0]) / (aabb[1] - aabb[0])"""

    def __init__(self, density: HashMLP, color: HashMLP, feature: HashMLP, world_to_nerf=None, contraction: bool = True, aabb=None,
                 average_init_density: float = 1.0):
        if not (density.device == color.device == feature.device):
            raise ValueError("FeatureFieldQuery: the three networks must live on one device")
        if density.out_dim < 2 or density.out_dim > 63 or density.n_extra or density.out_activation or not len(density.levels):
            raise ValueError(f"FeatureFieldQuery: the density net must take positions alone and give 2..63 linear outputs, got {density.out_dim}")
        if len(color.levels) or color.n_frequencies or color.n_extra != density.out_dim - 1 or color.out_dim != 3:
            raise ValueError(f"FeatureFieldQuery: the colour head must take the {density.out_dim - 1} geometry columns alone and give 3 outputs")
        if feature.n_extra or not len(feature.levels):
            raise ValueError("FeatureFieldQuery: the feature net takes positions alone")
        self.density, self.color, self.feature, self.device = density, color, feature, density.device
        a = np.eye(4)[:3] if world_to_nerf is None else np.asarray(world_to_nerf, np.float64)[:3]
        if a.shape != (3, 4):
            raise ValueError(f"FeatureFieldQuery: world_to_nerf must be (3, 4) or (4, 4), got {np.shape(world_to_nerf)}")
        self.world_to_nerf = a.astype(np.float32)
        self.contraction = bool(contraction)
        if not self.contraction and aabb is None:
            raise ValueError("FeatureFieldQuery: aabb is needed without contraction")
        self.aabb = np.asarray([[-1.0] * 3, [1.0] * 3] if aabb is None else aabb, np.float32).reshape(2, 3)
        if not self.contraction and not np.all(self.aabb[1] > self.aabb[0]):
            raise ValueError("FeatureFieldQuery: empty aabb")
        self.average_init_density = float(average_init_density)
        self.feature_dim = feature.out_dim

    # ---- constructors ----
    @classmethod
    def from_arrays(cls, density: Mapping, color: Mapping, feature: Mapping, world_to_nerf=None, contraction: bool = True, aabb=None,
                    average_init_density: float = 1.0, device="cuda:0") -> "FeatureFieldQuery":
        """Explicit tables and matrices: density / feature = dict(levels, table, weights, biases=None, n_frequencies=0), color =
        dict(weights, biases=None) with the constant inputs already folded (fold_color_head)."""
        d = HashMLP(density["levels"], density["table"], density["weights"], density.get("biases"), density.get("n_frequencies", 0), device=device)
        f = HashMLP(feature["levels"], feature["table"], feature["weights"], feature.get("biases"), feature.get("n_frequencies", 0), device=device)
        c = HashMLP(None, None, color["weights"], color.get("biases"), n_extra=d.out_dim - 1, out_activation="sigmoid", device=device)
        return cls(d, c, f, world_to_nerf, contraction, aabb, average_init_density)

    @classmethod
    def from_nerfstudio_state_dict(cls, state_dict: Mapping, config: Mapping, device="cuda:0") -> "FeatureFieldQuery":
        """The torch-implementation keys of a nerfacto field (mlp.py:271-292: Sequential(HashEncoding, MLP)):
            {field}.mlp_base.model.0.hash_table, {field}.mlp_base.model.1.layers.N.{weight,bias}, {field}.mlp_head.layers.N.{weight,bias},
            {field}.embedding_appearance.embedding.weight
        and for the feature net either the same pair under {feature}.field.0 / {feature}.field.1 or a tiny-cuda-nn vector
        {feature}.field.params (split_tcnn_params).  config: field_prefix ("field"), feature_prefix ("feature_field"); density =
        dict(num_levels, base_res, max_res, log2_hashmap_size) and feature = dict(num_levels, start_res, max_res,
        log2_hashmap_size, features_per_level, pe_n_freq, num_layers [hidden layers], feature_dim); sh_levels (4), sh_direction
        ((0.5, 0.5, 0.5): the torch SHEncoding sees get_normalized_directions(0)); use_average_appearance_embedding (False);
        world_to_nerf, contraction (True), aabb, average_init_density (1.0)."""
        sd = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in state_dict.items()}
        fp, qp = config.get("field_prefix", "field"), config.get("feature_prefix", "feature_field")

        def layers(prefix):
            ws, bs, i = [], [], 0
            while f"{prefix}.layers.{i}.weight" in sd:
                ws.append(sd[f"{prefix}.layers.{i}.weight"])
                bs.append(sd.get(f"{prefix}.layers.{i}.bias"))
                i += 1
            if not ws:
                raise KeyError(f"from_nerfstudio_state_dict: no '{prefix}.layers.0.weight' in the state dict")
            return ws, bs

        dc = config["density"]
        d_levels, d_rows = nerfstudio_levels(dc["num_levels"], dc["base_res"], dc["max_res"], dc["log2_hashmap_size"])
        d_table = sd[f"{fp}.mlp_base.model.0.hash_table"]
        if d_table.shape[0] != d_rows:
            raise ValueError(f"from_nerfstudio_state_dict: the density hash table has {d_table.shape[0]} rows, the config implies {d_rows}")
        dw, db = layers(f"{fp}.mlp_base.model.1")
        density = HashMLP(d_levels, d_table, dw, db, device=device)
        n_geo = density.out_dim - 1
        cw, cb = layers(f"{fp}.mlp_head")
        sh_levels = int(config.get("sh_levels", 4))
        emb = sd.get(f"{fp}.embedding_appearance.embedding.weight")
        appearance = None
        if emb is not None:
            appearance = emb.astype(np.float64).mean(axis=0) if config.get("use_average_appearance_embedding", False) else np.zeros(emb.shape[1])
        cw, cb = fold_color_head(cw, cb, sh_levels ** 2, n_geo, sh_components(sh_levels, config.get("sh_direction", (0.5, 0.5, 0.5))), appearance)
        color = HashMLP(None, None, cw, cb, n_extra=n_geo, out_activation="sigmoid", device=device)
        fc = config["feature"]
        n_freq = int(fc.get("pe_n_freq", 0))
        if f"{qp}.field.params" in sd:
            growth = growth_factor(fc["num_levels"], fc["start_res"], fc["max_res"])
            f_levels, f_rows = tcnn_levels(fc["num_levels"], fc["start_res"], growth, fc["log2_hashmap_size"])
            F = int(fc["features_per_level"])
            fw, fb, f_table = split_tcnn_params(sd[f"{qp}.field.params"], fc["num_levels"] * F + 6 * n_freq, int(fc["num_layers"]), int(fc["feature_dim"]),
                                                f_rows, F)
        else:
            f_levels, f_rows = nerfstudio_levels(fc["num_levels"], fc["start_res"], fc["max_res"], fc["log2_hashmap_size"])
            f_table = sd[f"{qp}.field.0.hash_table"]
            if f_table.shape[0] != f_rows:
                raise ValueError(f"from_nerfstudio_state_dict: the feature hash table has {f_table.shape[0]} rows, the config implies {f_rows}")
            fw, fb = layers(f"{qp}.field.1")
        feature = HashMLP(f_levels, f_table, fw, fb, n_frequencies=n_freq, device=device)
        return cls(density, color, feature, config.get("world_to_nerf"), config.get("contraction", True), config.get("aabb"),
                   config.get("average_init_density", 1.0))

    @classmethod
    def from_tcnn_params(cls, params: Mapping, config: Mapping, device="cuda:0") -> "FeatureFieldQuery":
        """params: dict(density=, color=, feature=) of flat tiny-cuda-nn `params` vectors (mlp_base.model.params, mlp_head.
        tcnn_encoding.params, feature_field.field.params), each in the layout split_tcnn_params documents.  config as
        from_nerfstudio_state_dict's, plus density.features_per_level (2), density.num_layers / color.num_layers [hidden layers],
        geo_feat_dim (15), appearance (None or the constant embedding vector), sh_direction ((0, 0, 0): tiny-cuda-nn's
        SphericalHarmonics maps its [0, 1] input to 2 x - 1)."""
        dc, fc, cc = config["density"], config["feature"], config.get("color", {})
        n_geo = int(config.get("geo_feat_dim", 15))
        Fd = int(dc.get("features_per_level", 2))
        d_levels, d_rows = tcnn_levels(dc["num_levels"], dc["base_res"], growth_factor(dc["num_levels"], dc["base_res"], dc["max_res"]), dc["log2_hashmap_size"])
        dw, db, d_table = split_tcnn_params(params["density"], dc["num_levels"] * Fd, int(dc.get("num_layers", 1)), 1 + n_geo, d_rows, Fd)
        density = HashMLP(d_levels, d_table, dw, db, device=device)
        sh_levels = int(config.get("sh_levels", 4))
        appearance = config.get("appearance")
        n_app = 0 if appearance is None else len(appearance)
        cw, cb, _ = split_tcnn_params(params["color"], sh_levels ** 2 + n_geo + n_app, int(cc.get("num_layers", 2)), 3)
        cw, cb = fold_color_head(cw, cb, sh_levels ** 2, n_geo, sh_components(sh_levels, config.get("sh_direction", (0.0, 0.0, 0.0))), appearance)
        color = HashMLP(None, None, cw, cb, n_extra=n_geo, out_activation="sigmoid", device=device)
        n_freq, Ff = int(fc.get("pe_n_freq", 0)), int(fc["features_per_level"])
        f_levels, f_rows = tcnn_levels(fc["num_levels"], fc["start_res"], growth_factor(fc["num_levels"], fc["start_res"], fc["max_res"]), fc["log2_hashmap_size"])
        fw, fb, f_table = split_tcnn_params(params["feature"], fc["num_levels"] * Ff + 6 * n_freq, int(fc["num_layers"]), int(fc["feature_dim"]), f_rows, Ff)
        feature = HashMLP(f_levels, f_table, fw, fb, n_frequencies=n_freq, device=device)
        return cls(density, color, feature, config.get("world_to_nerf"), config.get("contraction", True), config.get("aabb"),
                   config.get("average_init_density", 1.0))

    # ---- the descriptor ----
    def desc(self, min_bounds=(0.0, 0.0, 0.0), voxel_size: float = 1.0, shape=(1, 1, 1), alpha_weighted: bool = True, axes=None) -> FieldVoxelizeDesc:
        v = FieldVoxelizeDesc()
        if axes is not None:
            v.d_axis_x, v.d_axis_y, v.d_axis_z = (a.data_ptr() for a in axes)
        self.density.fill(v.density)
        self.color.fill(v.color)
        self.feature.fill(v.feature)
        v.min_bounds = (C.c_double * 3)(*[float(x) for x in min_bounds])
        v.voxel_size = float(voxel_size)
        v.d, v.h, v.w = (int(s) for s in shape)
        v.contraction, v.alpha_weighted, v.average_init_density = int(self.contraction), int(bool(alpha_weighted)), self.average_init_density
        v.world_to_nerf = (C.c_float * 12)(*self.world_to_nerf.reshape(-1).tolist())
        v.aabb = (C.c_float * 6)(*self.aabb.reshape(-1).tolist())
        return v

    # ---- FeatureFieldAdapter's surface ----
    def _points(self, world_points, delta=0.0, feature=False, alpha=False, rgb=False, density=False):
        if not torch.is_tensor(world_points) or world_points.device != self.device:
            raise _lib.PixieHipError(f"FeatureFieldQuery: world_points must be a tensor on {self.device} (no CPU fallback)")
        if world_points.shape[-1] != 3:
            raise ValueError(f"FeatureFieldQuery: world_points must be (..., 3), got {tuple(world_points.shape)}")
        lead = tuple(world_points.shape[:-1])
        pts = world_points.reshape(-1, 3).to(torch.float32).contiguous()
        n = int(pts.shape[0])
        new = lambda c: torch.empty((n, c), dtype=torch.float32, device=self.device)
        out = {"feature": new(self.feature_dim) if feature else None, "alpha": new(1) if alpha else None, "rgb": new(3) if rgb else None,
               "density": new(1) if density else None}
        ptr = lambda t: t.data_ptr() if t is not None else None
        lib = _lib.load()
        with torch.cuda.device(self.device):
            check(lib.pixie_field_query_points(C.byref(self.desc()), pts.data_ptr(), n, float(delta), ptr(out["feature"]), ptr(out["alpha"]),
                                               ptr(out["rgb"]), ptr(out["density"]), _lib.current_stream_ptr()), "pixie_field_query_points")
        return {k: t.reshape(*lead, t.shape[1]) for k, t in out.items() if t is not None}

    def __call__(self, world_points) -> Dict[str, torch.Tensor]:
        out = self._points(world_points, feature=True, density=True)
        return {"density": out["density"], "feature": out["feature"]}

    forward = __call__

    def get_density(self, world_points) -> torch.Tensor:
        return self._points(world_points, density=True)["density"]

    def get_alpha(self, world_points, delta: float) -> torch.Tensor:
        return self._points(world_points, delta=delta, alpha=True)["alpha"]

    def get_rgb(self, world_points) -> torch.Tensor:
        return self._points(world_points, rgb=True)["rgb"]

    # ---- the fused lattice call ----
    def voxelize(self, min_bounds: Sequence[float], max_bounds: Sequence[float], voxel_size: float, alpha_weighted: bool = True,
                 return_density: bool = False, return_alpha32: bool = False):
        """(features (D, H, W, C), alphas (D, H, W, 1), rgb (D, H, W, 3)) float16 device tensors on the lattice of dense_voxel_grid
        (initial_proposals.py:18-27): torch.arange(min, max, voxel_size) per axis, evaluated by torch on the host as the reference
        evaluates it (three small arrays; the closed form float32(min + i voxel_size) is up to a few ulps off what the CPU's
        vectorised arange gives).  One pixie_field_voxelize call.  With return_density / return_alpha32 the float32 density /
        alpha grids (D, H, W) follow."""
        dev = self.device
        host_axes = lattice_axes(min_bounds, max_bounds, voxel_size)
        shape = tuple(len(a) for a in host_axes)
        axes = [a.to(dev) for a in host_axes]
        D, H, W = shape
        features = torch.empty((D, H, W, self.feature_dim), dtype=torch.float16, device=dev)
        alphas = torch.empty((D, H, W, 1), dtype=torch.float16, device=dev)
        rgb = torch.empty((D, H, W, 3), dtype=torch.float16, device=dev)
        density = torch.empty((D, H, W), dtype=torch.float32, device=dev) if return_density else None
        scratch = torch.empty((D, H, W), dtype=torch.float32, device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            check(lib.pixie_field_voxelize(C.byref(self.desc(min_bounds, voxel_size, shape, alpha_weighted, axes)), features.data_ptr(), alphas.data_ptr(),
                                           rgb.data_ptr(), density.data_ptr() if density is not None else None, scratch.data_ptr(),
                                           _lib.current_stream_ptr()), "pixie_field_voxelize")
        out = (features, alphas, rgb)
        if return_density:
            out += (density,)
        if return_alpha32:
            out += (scratch,)
        return out


def lattice_axes(min_bounds, max_bounds, voxel_size):
    """dense_voxel_grid's three axes (initial_proposals.py:22-23), by the same torch.arange calls on the host"""
    axes = [torch.arange(lo, hi, voxel_size) for lo, hi in zip(min_bounds, max_bounds)]
    if min(len(a) for a in axes) < 1:
        raise ValueError(f"field_query: empty lattice {[len(a) for a in axes]}")
    return [a.to(torch.float32) for a in axes]


def _split_bounds(bounds):
    return tuple(b[0] for b in bounds), tuple(b[1] for b in bounds)


MASK_ARGS = {"alpha_threshold_for_mask": "alpha_threshold", "gray_threshold_for_mask": "gray_threshold", "run_outlier_filter": "run_outlier_filter",
             "nb_neighbors": "nb_neighbors", "std_ratio": "std_ratio", "min_cluster_pts": "min_cluster_pts", "eps_multiplier": "eps_multiplier"}


def _mask_kwargs(mask_args):
    unknown = set(mask_args) - set(MASK_ARGS)
    if unknown:
        raise TypeError(f"extract_clip_voxel_grid: unknown arguments {sorted(unknown)}")
    return {MASK_ARGS[k]: v for k, v in mask_args.items()}


def extract_clip_voxel_grid(field: FeatureFieldQuery, output_path: str, bounds=((-0.5, 0.5), (-0.5, 0.5), (-0.5, 0.5)), voxel_size: float = 0.01,
                            alpha_weighted: bool = True, **mask_args) -> str:
    """voxelize.py:17-141 with the loaded field in place of scene_path: one fused call, then the reference's files -- output_path
    (.npz metadata, the keys of :162-171), *_features.npy, *_alphas.npy, *_rgb.npy and *_mask.npy (create_occupancy_mask).
    mask_args: alpha_threshold_for_mask, gray_threshold_for_mask, run_outlier_filter, nb_neighbors, std_ratio, min_cluster_pts,
    eps_multiplier, with the reference's defaults.  Returns output_path."""
    from .occupancy import create_occupancy_mask
    kw = _mask_kwargs(mask_args)
    min_bounds, max_bounds = _split_bounds(bounds)
    features, alphas, rgb = field.voxelize(min_bounds, max_bounds, voxel_size, alpha_weighted)
    os.makedirs(os.path.dirname(os.path.abspath(output_path)), exist_ok=True)
    np.savez_compressed(output_path, min_bounds=min_bounds, max_bounds=max_bounds, voxel_size=voxel_size, feature_dim=field.feature_dim,
                        grid_shape=tuple(features.shape[:3]), alpha_weighted=alpha_weighted,
                        alpha_threshold_for_mask=mask_args.get("alpha_threshold_for_mask", 0.01))
    np.save(output_path.replace(".npz", "_features.npy"), features.cpu().numpy())
    np.save(output_path.replace(".npz", "_alphas.npy"), alphas.cpu().numpy())
    np.save(output_path.replace(".npz", "_rgb.npy"), rgb.cpu().numpy())
    create_occupancy_mask(output_path, alphas, rgb, voxel_size, min_bounds, device=field.device, **kw)
    return output_path


def voxelize_to_device(field: FeatureFieldQuery, bounds=((-0.5, 0.5), (-0.5, 0.5), (-0.5, 0.5)), voxel_size: float = 0.01,
                       alpha_weighted: bool = True, **mask_args):
    """(feat_grid (1, C, D, H, W) float32, mask (D, H, W) bool, min_bounds, max_bounds) as neural_scene_rollout takes them, nothing
    written to disk: the float16 grid is widened exactly as load_voxel_grid widens the file."""
    from .occupancy import occupancy_mask
    from .voxel_grid import load_voxel_grid
    kw = _mask_kwargs(mask_args)
    min_bounds, max_bounds = _split_bounds(bounds)
    features, alphas, rgb = field.voxelize(min_bounds, max_bounds, voxel_size, alpha_weighted)
    mask = occupancy_mask(alphas, rgb, voxel_size, min_bounds, device=field.device, **kw)
    return load_voxel_grid(features, device=field.device), mask, min_bounds, max_bounds
