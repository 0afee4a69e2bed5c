"""Language-query part segmentation and the material grid on the device (material_mode=vlm).

Mirrors pixie/voxel/segmentation.py: `run_clip` / `clip_part_segmentation` (:98-168) score every masked voxel of the CLIP feature
grid against the text embeddings of the part names, `local_post_process_segmentation` (:190-226) re-labels each voxel by the vote
of its 200 nearest neighbours (a Python loop over a k-d tree), and `save_segmented_point_cloud` (:231-472) writes
segmented_semantics.ply -- the file gs_simulation.py --point_cloud_path reads in that mode -- and material_grid.npy, the target the
two U-Nets are trained on.  Here one pixie_part_segmentation call (HIP, pixie_amd/csrc/part_segmentation.hip) does the compute on
the tensors' device and torch's current stream, without a stream synchronise or a host read-back.  (With smooth_k the wrapper reads
the mask's sum first, to raise where the k-d tree would; that is its one synchronise.)

    part_segmentation(features, mask, query_embeddings, ...)   -> PartSegmentation (dense grids on the device)
    material_grid(seg, props, background_id=7)                 -> (D, H, W, 4) float32 device tensor
    segment_scene(grid_feature_path, material_props, ...)      -> writes the reference's files, returns its metrics dict

CLIP itself is not here: part names reach the call as a (K, C) embedding matrix, or through `encode`, a callable from the list of
names to that matrix.  Limits: K <= 32 parts, C a multiple of 8 and <= 2048, K C 4 <= 96 KB, smooth_k <= 255.

The vote's last shell.  On the lattice the k nearest voxels are whole shells of integer squared offset and only the last shell is
taken in part; which of its members a k-d tree returns is an artefact of its traversal.  Here the rule is fixed: neighbours are
ordered by (integer squared offset, C-order linear index of the neighbour voxel) and the first k are taken.
`connected_component_cleanup` is defined in the reference but never called, and is not restated.  There is no CPU compute path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import PartSegDesc, check
from .occupancy import _lattice_spacing
from .ply_io import write_ply

MAX_PARTS, MAX_CHANNELS, MAX_QUERY_BYTES, MAX_SMOOTH_K = 32, 2048, 96 * 1024, 255
REFERENCE_SMOOTH_K = 200                                   # local_post_process_segmentation's default
MATERIAL_DEFAULTS = {"density": 200, "E": 2e6, "nu": 0.4, "material_id": 0}   # segmentation.py:334-337
# matplotlib's qualitative 'tab10' map, kept as constants (the reference: plt.colormaps['tab10'](i % 10))
TAB10 = tuple(tuple(c / 255.0 for c in rgb) for rgb in (
    (31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189),
    (140, 86, 75), (227, 119, 194), (127, 127, 127), (188, 189, 34), (23, 190, 207)))
VERTEX_DTYPE = [("x", "f4"), ("y", "f4"), ("z", "f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"), ("alpha", "u1"),
                ("part_label", "i4"), ("density", "f4"), ("E", "f4"), ("nu", "f4"), ("material_id", "i4")]   # segmentation.py:381-389


class PartSegmentation:
    """What one part_segmentation call left on the device.

    label_grid     (D, H, W) int8, the stage-A label, -1 outside the mask
    score_grid     (D, H, W) float32, softmax(sim / T)[label], NaN outside the mask
    smoothed_grid  (D, H, W) int8 after the k-nearest-neighbour vote, or None without smooth_k
    final_grid     smoothed_grid if the vote ran, else label_grid
    material_grid  (D, H, W, 4) float32 if `props` was given, else None
    part_labels    (n,) int64 and part_scores (n,) float32 in the mask's C order, as features_flat[linear_mask] orders them; the
                   labels are final_grid's, the scores stay stage A's (the reference keeps them too).  Built on first use by one
                   grid[mask] gather each, the only synchronise.
    counts         list of K ints, voxels per part by the stage-A labels (clip_part_segmentation's metrics); the first read
                   synchronises.  n_masked and slow_path_voxels come with it."""

    def __init__(self, mask, label_grid, score_grid, smoothed_grid, material, counts, n_parts):
        self.mask, self.label_grid, self.score_grid, self.smoothed_grid, self.material_grid = mask, label_grid, score_grid, smoothed_grid, material
        self.n_parts = n_parts
        self._counts, self._host, self._labels, self._scores = counts, None, None, None

    @property
    def final_grid(self):
        return self.smoothed_grid if self.smoothed_grid is not None else self.label_grid

    @property
    def part_labels(self):
        if self._labels is None:
            self._labels = self.final_grid[self.mask].to(torch.int64)
        return self._labels

    @property
    def part_scores(self):
        if self._scores is None:
            self._scores = self.score_grid[self.mask]
        return self._scores

    def _read(self):
        if self._host is None:
            self._host = self._counts.cpu().tolist()
        return self._host

    @property
    def counts(self):
        return self._read()[:self.n_parts]

    @property
    def n_masked(self):
        return self._read()[MAX_PARTS]

    @property
    def slow_path_voxels(self):
        return self._read()[MAX_PARTS + 1]


def _device_tensor(x, what):
    if not torch.is_tensor(x) or x.device.type != "cuda":
        raise _lib.PixieHipError(f"part_segmentation: {what} must be a tensor on a HIP device (no CPU fallback)")
    return x.detach()


def _small_matrix(x, dev, cols, what):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not torch.is_tensor(t) or t.dim() != 2 or (cols is not None and t.shape[1] != cols):
        raise ValueError(f"part_segmentation: {what} must be a 2-D array{'' if cols is None else f' with {cols} columns'}")
    if t.dtype != torch.float32:
        raise ValueError(f"part_segmentation: {what} must be float32, got {t.dtype}")
    return t.detach().to(dev).contiguous()


def _check_axes(host_axes):
    """The vote works on index offsets, so the coordinates must be a lattice: occupancy._lattice_spacing's rule (every axis ascends,
    the axes' mean steps agree to 1e-3) applied to every single step as well, against the spacing it returns."""
    try:
        spacing = _lattice_spacing(host_axes, 1.0)
    except ValueError as e:
        raise ValueError(str(e).replace("occupancy_mask", "part_segmentation")) from None
    for x in host_axes:
        steps = torch.diff(x.double())
        if len(steps) and (float(steps.min()) * (1.0 + 1e-3) < spacing or float(steps.max()) > spacing * (1.0 + 1e-3)):
            raise ValueError("part_segmentation: every axis must ascend with one spacing")


def part_segmentation(features, mask, query_embeddings, *, softmax_temperature: float = 0.1, smooth_k: Optional[int] = None, axes=None,
                      props=None, background_id: float = 7):
    """features (D, H, W, C) float16 and mask (D, H, W) bool, both device tensors that stay where they are; query_embeddings (K, C)
    float32, un-normalised (numpy or tensor) -> PartSegmentation.

    sim_j = <f, q_j> / (|f| |q_j|) in float32 on the widened row; label = argmax_j sim_j, ties to the lowest index as torch.argmax;
    score = 1 / sum_j exp((sim_j - sim_max) / T) = softmax(sim / T)[label].  A row of zero norm gets label 0 and score NaN, which is
    what torch's expression gives.

    smooth_k (the reference: 200) turns on the k-nearest-neighbour vote of use_spatial_smoothing: every vote reads the stage-A
    labels, equal counts go to the smallest label as scipy.stats.mode does, the last shell is taken by the rule in the module
    docstring.  `axes`: the three coordinate arrays on the host; when given they must ascend with a single spacing, since the vote
    works on index offsets.  Fewer masked voxels than smooth_k raise ValueError (sklearn's KDTree.query raises too); that check
    reads the mask's sum on the host, so with smooth_k this wrapper synchronises once before the call -- the C call itself never
    does, and without smooth_k nothing here does.  `props` (K, 4) float32 = density, E, nu, material_id per part fuses material_grid into the call."""
    f, m = _device_tensor(features, "features"), _device_tensor(mask, "mask")
    dev = f.device
    if m.device != dev:
        raise ValueError("part_segmentation: features and mask are on different devices")
    if f.dim() != 4 or f.dtype != torch.float16:
        raise ValueError(f"part_segmentation: features must be (D, H, W, C) float16, got {tuple(f.shape)} {f.dtype}")
    D, H, W, channels = (int(s) for s in f.shape)
    if tuple(m.shape) != (D, H, W) or m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"part_segmentation: mask must be {(D, H, W)} bool, got {tuple(m.shape)} {m.dtype}")
    if channels % 8 != 0 or not 8 <= channels <= MAX_CHANNELS:
        raise ValueError(f"part_segmentation: C = {channels}, a multiple of 8 up to {MAX_CHANNELS} is supported")
    q = _small_matrix(query_embeddings, dev, channels, "query_embeddings")
    n_parts = int(q.shape[0])
    if not 1 <= n_parts <= MAX_PARTS:
        raise ValueError(f"part_segmentation: K = {n_parts} parts, 1 to {MAX_PARTS} are supported")
    if n_parts * channels * 4 > MAX_QUERY_BYTES:
        raise ValueError(f"part_segmentation: K C 4 = {n_parts * channels * 4} bytes of queries exceed {MAX_QUERY_BYTES}")
    if not softmax_temperature > 0.0:
        raise ValueError(f"part_segmentation: softmax_temperature {softmax_temperature} is not positive")
    p = _small_matrix(props, dev, 4, "props") if props is not None else None
    if p is not None and p.shape[0] != n_parts:
        raise ValueError(f"part_segmentation: props has {p.shape[0]} rows for {n_parts} parts")
    f, m = f.contiguous(), m.contiguous()
    mask_bool = m if m.dtype == torch.bool else m != 0
    vote_k = 0
    if smooth_k is not None:
        vote_k = int(smooth_k)
        if not 1 <= vote_k <= MAX_SMOOTH_K:
            raise ValueError(f"part_segmentation: smooth_k = {smooth_k}, 1 to {MAX_SMOOTH_K} are supported")
        if axes is not None:
            if any(torch.is_tensor(x) and x.device.type != "cpu" for x in axes):
                raise ValueError("part_segmentation: axes must be host arrays (their spacing is checked on the host)")
            host_axes = [torch.as_tensor(np.asarray(x), dtype=torch.float32) for x in axes]
            if [len(x) for x in host_axes] != [D, H, W]:
                raise ValueError(f"part_segmentation: axes of {[len(x) for x in host_axes]} points for a grid of {(D, H, W)}")
            _check_axes(host_axes)
        n_masked = int(mask_bool.sum())
        if n_masked < vote_k:
            raise ValueError(f"part_segmentation: {n_masked} masked voxels are fewer than smooth_k = {vote_k}")

    lib = _lib.load()
    desc = PartSegDesc()
    desc.d_features, desc.d_mask, desc.d_queries = f.data_ptr(), m.data_ptr(), q.data_ptr()
    desc.d_props = p.data_ptr() if p is not None else None
    desc.d, desc.h, desc.w, desc.channels, desc.n_parts, desc.vote_k = D, H, W, channels, n_parts, vote_k
    desc.temperature, desc.background_id = float(softmax_temperature), float(background_id)
    with torch.cuda.device(dev):
        need = lib.pixie_part_seg_scratch_bytes(C.byref(desc))
        if need < 0:
            check(1, "pixie_part_seg_scratch_bytes", lib=lib)
        labels = torch.empty((D, H, W), dtype=torch.int8, device=dev)
        scores = torch.empty((D, H, W), dtype=torch.float32, device=dev)
        voted = torch.empty((D, H, W), dtype=torch.int8, device=dev) if vote_k else None
        material = torch.empty((D, H, W, 4), dtype=torch.float32, device=dev) if p is not None else None
        counts = torch.empty(_lib.PART_SEG_COUNTS, dtype=torch.int64, device=dev)
        scratch = torch.empty(max(int(need), 16), dtype=torch.uint8, device=dev)
        check(lib.pixie_part_segmentation(C.byref(desc), C.c_void_p(labels.data_ptr()), C.c_void_p(scores.data_ptr()),
                                          C.c_void_p(voted.data_ptr() if voted is not None else 0),
                                          C.c_void_p(material.data_ptr() if material is not None else 0),
                                          C.c_void_p(counts.data_ptr()), C.c_void_p(scratch.data_ptr()), _lib.current_stream_ptr()),
              "pixie_part_segmentation", lib=lib)
        # queries and scratch go back to torch's caching allocator here; launches queued on this stream are ordered before any reuse
    return PartSegmentation(mask_bool, labels, scores, voted, material, counts, n_parts)


def material_grid(seg: PartSegmentation, props, background_id: float = 7):
    """(D, H, W, 4) float32 device tensor: props[label] = density, E, nu, material_id on the mask (the voted labels when the vote
    ran), [0, 0, 0, background_id] elsewhere (segmentation.py:429-452)."""
    grid = seg.final_grid
    dev = grid.device
    p = _small_matrix(props, dev, 4, "props")
    if p.shape[0] != seg.n_parts:
        raise ValueError(f"material_grid: props has {p.shape[0]} rows for {seg.n_parts} parts")
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = torch.empty(tuple(grid.shape) + (4,), dtype=torch.float32, device=dev)
        check(lib.pixie_part_material_grid(C.c_void_p(grid.data_ptr()), C.c_void_p(p.data_ptr()), seg.n_parts, grid.numel(), float(background_id),
                                           C.c_void_p(out.data_ptr()), _lib.current_stream_ptr()), "pixie_part_material_grid", lib=lib)
    return out


def props_matrix(material_props: Dict[str, Dict[str, float]]) -> np.ndarray:
    """(K, 4) float32 rows density, E, nu, material_id in the dictionary's order, with the defaults of segmentation.py:334-337."""
    return np.array([[props.get(key, MATERIAL_DEFAULTS[key]) for key in ("density", "E", "nu", "material_id")]
                     for props in material_props.values()], dtype=np.float32).reshape(len(material_props), 4)


def _colour_bytes(rgba: np.ndarray) -> np.ndarray:
    return (rgba.astype(np.float32) * 255).astype(np.uint8)              # segmentation.py:344,378: truncation, not rounding


def segment_scene(grid_feature_path: str, material_props: Dict[str, Dict[str, float]], query_embeddings=None, *,
                  encode: Optional[Callable[[Sequence[str]], object]] = None, output_dir: str, use_spatial_smoothing: bool = False,
                  background_id: int = 7, rgb=None, softmax_temperature: float = 0.1, device="cuda:0") -> Dict[str, int]:
    """segmentation.py's __main__ for the files extract_clip_voxel_grid leaves next to `grid_feature_path` (<stem>.npz with
    min_bounds, max_bounds, grid_shape; <stem>_features.npy (D, H, W, C) float16; <stem>_mask.npy).  The part names are the keys
    of `material_props` (a dictionary under "material_dict" is unwrapped); their embeddings are `query_embeddings` (K, C) in that
    order, or encode(names).  Writes into output_dir: part_labels.npy (int64, the mask's C order), segmented_semantics.ply and
    segmented_rgb.ply (properties of :381-403), material_grid.npy and density_grid.npy, E_grid.npy, nu_grid.npy,
    material_id_grid.npy (:463-471).  Returns the metrics dict of :175-181 (with "initial" and "masked_voxels" of :61,85).

    Coordinates are torch.linspace(min, max, n) per axis (:70-74).  The semantic colours are tab10's; segmented_rgb.ply takes the
    caller's `rgb` (n, 3) in [0, 1] in the mask's C order and is white without it, as the reference's branch without an original
    cloud -- its nearest-vertex colour lookup in clip_features_pc.ply is not restated (that file is visualisation only)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.PixieHipError("segment_scene runs on a HIP device only (no CPU fallback)")
    if "material_dict" in material_props:
        material_props = material_props["material_dict"]
    names = list(material_props.keys())
    if (query_embeddings is None) == (encode is None):
        raise ValueError("segment_scene: give query_embeddings or encode, not both")
    if query_embeddings is None:
        query_embeddings = encode(names)
    q = query_embeddings.detach().float() if torch.is_tensor(query_embeddings) else np.asarray(query_embeddings, np.float32)
    if q.shape[0] != len(names):
        raise ValueError(f"segment_scene: {q.shape[0]} embeddings for {len(names)} part names")
    meta = np.load(grid_feature_path)
    min_bounds, max_bounds, grid_shape = meta["min_bounds"], meta["max_bounds"], meta["grid_shape"]
    features = np.load(grid_feature_path.replace(".npz", "_features.npy"))
    if features.dtype != np.float16:
        raise ValueError(f"segment_scene: the feature grid must be float16 as voxelize.py writes it, got {features.dtype}")
    mask_path = grid_feature_path.replace(".npz", "_mask.npy")
    if not os.path.exists(mask_path):
        raise FileNotFoundError(f"Mask not found at {mask_path}. Please run voxelization first.")
    mask_np = np.load(mask_path).astype(bool)
    axes = [torch.linspace(float(min_bounds[a]), float(max_bounds[a]), int(grid_shape[a]), device=dev) for a in range(3)]
    props = props_matrix(material_props)

    seg = part_segmentation(torch.from_numpy(features).to(dev), torch.from_numpy(mask_np).to(dev), q, softmax_temperature=softmax_temperature,
                            smooth_k=REFERENCE_SMOOTH_K if use_spatial_smoothing else None, axes=[a.cpu() for a in axes],
                            props=props, background_id=background_id)
    idx = torch.nonzero(seg.mask)
    coords = torch.stack([axes[a][idx[:, a]] for a in range(3)], dim=1).cpu().numpy()
    labels = seg.part_labels.cpu().numpy()
    grid = seg.material_grid.cpu().numpy()
    metrics = {"initial": np.prod(grid_shape), "masked_voxels": int(seg.n_masked), "num_parts": len(names)}
    for i, name in enumerate(names):
        metrics[f"part_{i}_{name}"] = seg.counts[i]

    os.makedirs(output_dir, exist_ok=True)
    np.save(os.path.join(output_dir, "part_labels.npy"), labels)
    n = len(labels)
    semantic = np.zeros((n, 4), dtype=np.float32)
    for i in range(len(names)):
        semantic[labels == i] = np.array(TAB10[i % len(TAB10)] + (1.0,))
    colours = np.ones((n, 4), dtype=np.float32)
    if rgb is not None:
        rgb = rgb.detach().cpu().numpy() if torch.is_tensor(rgb) else np.asarray(rgb)
        if rgb.shape != (n, 3):
            raise ValueError(f"segment_scene: rgb must be {(n, 3)}, got {rgb.shape}")
        colours[:, :3] = rgb
    for fname, rgba in (("segmented_rgb.ply", colours), ("segmented_semantics.ply", semantic)):
        vertex = np.zeros(n, dtype=VERTEX_DTYPE)
        vertex["x"], vertex["y"], vertex["z"] = coords[:, 0], coords[:, 1], coords[:, 2]
        u8 = _colour_bytes(rgba)
        vertex["red"], vertex["green"], vertex["blue"], vertex["alpha"] = u8[:, 0], u8[:, 1], u8[:, 2], u8[:, 3]
        vertex["part_label"] = labels
        vertex["density"], vertex["E"], vertex["nu"] = props[labels, 0], props[labels, 1], props[labels, 2]
        vertex["material_id"] = props[labels, 3].astype(np.int32)
        write_ply(os.path.join(output_dir, fname), vertex, text=False)
    np.save(os.path.join(output_dir, "material_grid.npy"), grid)
    for channel, fname in enumerate(("density_grid.npy", "E_grid.npy", "nu_grid.npy", "material_id_grid.npy")):
        np.save(os.path.join(output_dir, fname), grid[..., channel])
    return metrics
