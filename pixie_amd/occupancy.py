"""The occupancy mask on the device: density, gray, outlier and cluster filters.

Mirrors pixie/voxel/voxelize.py `_create_occupancy_mask` (:188-263) and `compute_occupancy_point_cloud` (:266-406), which threshold
on the host and hand the voxels to Open3D (`remove_statistical_outlier`, `cluster_dbscan`; f3rm_robot/optimize.py:44-89
`remove_floating_clusters`).  Here one pixie_occupancy_mask call (HIP, pixie_amd/csrc/occupancy.hip) does all of it on the tensors'
device and torch's current stream, without a stream synchronise or a host read-back; the counts stay on the device until the stats
object is asked for them.

    occupancy_mask(alphas, rgb, voxel_size, min_bounds, ...)   -> (D, H, W) bool device tensor [, OccupancyStats]
    create_occupancy_mask(output_path, alphas, rgb, ...)       -> writes <output_path minus .npz>_mask.npy (voxelize.py:256-262)
    occupancy_points(feature_grid_path, ...)                   -> (xyz, rgb, metrics) of compute_occupancy_point_cloud
    load_voxel_scene(npz_path, device, recompute_mask=False)   -> (feat_grid, mask, min_bounds, max_bounds) for neural_scene_rollout

Not pinned to Open3D: both filters are restated from its published algorithm (RemoveStatisticalOutliers, ClusterDBSCAN) on the
voxel lattice.  The one place where that algorithm differs from sklearn's DBSCAN (pixie_amd.material_field.dbscan_labels) is the
radius rule: Open3D's search keeps dist < radius, sklearn's dist <= radius.  Cluster ids are not returned; clusters are numbered
by ascending lowest core voxel in C order where a rule needs a "first".  There is no CPU compute path.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import OccupancyDesc, check
from .voxel_grid import load_voxel_grid

KEEP_RULES = {"non_noise": 0, "largest": 1}
COUNT_NAMES = ("after_density", "after_gray", "after_outlier_removal", "after_cluster_removal", "slow_path_voxels", "n_clusters")


class OccupancyStats:
    """What one occupancy_mask call left on the device.  Nothing is copied to the host until an attribute is read (the first read
    synchronises with the call): `counts` (dict of COUNT_NAMES), `cloud_mean`, `std`, `threshold` (= cloud_mean + std_ratio std) and
    `mean_dist`, the (D, H, W) float64 device tensor of every candidate's mean neighbour distance, NaN elsewhere.  With
    run_outlier_filter=False stage B did not run: the three statistics are NaN and `mean_dist` is None."""

    def __init__(self, counts, stats, mean_dist):
        self._counts, self._stats, self.mean_dist = counts, stats, mean_dist
        self._host = None

    def _read(self):
        if self._host is None:
            self._host = (self._counts.cpu().tolist(), self._stats.cpu().tolist())
        return self._host

    @property
    def counts(self):
        return dict(zip(COUNT_NAMES, self._read()[0]))

    @property
    def cloud_mean(self):
        return self._read()[1][0]

    @property
    def std(self):
        return self._read()[1][1]

    @property
    def threshold(self):
        return self._read()[1][2]


def reference_axes(shape: Sequence[int], voxel_size: float, min_bounds: Sequence[float]):
    """The coordinates of voxelize.py's grid: torch.arange(min, max, voxel_size) per axis (f3rm_robot/initial_proposals.py:18-27),
    i.e. float32(min + i voxel_size) evaluated in double, for the number of voxels the arrays have."""
    return [(torch.arange(int(n), dtype=torch.float64) * float(voxel_size) + float(lo)).to(torch.float32) for n, lo in zip(shape, min_bounds)]


def _lattice_spacing(axes, voxel_size: float) -> float:
    steps = [(float(a[-1]) - float(a[0])) / (len(a) - 1) for a in axes if len(a) > 1]
    if not steps:
        return float(voxel_size)
    if min(steps) <= 0.0 or max(steps) > min(steps) * (1.0 + 1e-3):
        raise ValueError(f"occupancy_mask: the three axes must ascend with one spacing, got {steps}")
    return sum(steps) / len(steps)


def _as_device_array(x, dev, what):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not torch.is_tensor(t):
        raise ValueError(f"occupancy_mask: {what} must be a numpy array or a tensor")
    if t.dtype not in (torch.float16, torch.float32):
        raise ValueError(f"occupancy_mask: {what} must be float16 or float32, got {t.dtype}")
    return t.detach().to(dev)


def occupancy_mask(alphas, rgb, voxel_size: float, min_bounds: Sequence[float] = (-0.5,) * 3, *, alpha_threshold: float = 0.01,
                   gray_threshold: float = 0.05, run_outlier_filter: bool = True, nb_neighbors: int = 50, std_ratio: float = 4.0,
                   min_cluster_pts: int = 10, eps_multiplier: float = 5.0, keep: str = "non_noise", return_stats: bool = False,
                   axes=None, device=None):
    """alphas (D, H, W) or (D, H, W, 1) and rgb (D, H, W, 3), float16 (what voxelize.py writes) or float32, numpy or tensor ->
    (D, H, W) bool tensor on the device; the defaults are extract_clip_voxel_grid's.

    A voxel is a candidate iff float32(alpha) > alpha_threshold and the float32 mean ((r + g) + b) / 3 > gray_threshold (both
    thresholds rounded to float32, as torch compares a float32 tensor with a Python number).  run_outlier_filter=False stops there
    (voxelize.py:252-253).  Otherwise statistical outlier removal (nb_neighbors, std_ratio) and DBSCAN with eps = voxel_size *
    eps_multiplier and min_cluster_pts follow; keep="non_noise" keeps every clustered voxel (voxelize.py:250), keep="largest" the
    biggest cluster, or everything if there is none (remove_floating_clusters).

    The voxel coordinates are rebuilt as the reference builds them (reference_axes) unless `axes` gives three ascending float32
    HOST arrays (numpy or CPU tensors; device tensors are refused) of one spacing.  `device`: where numpy / host inputs go (default cuda:0); device tensors stay where they are.
    Rounding: a voxel whose mean distance lies within 4 E + 1e-12 of the threshold (E: the axes' largest deviation from a uniform
    lattice) may fall on the other side than in a k-d tree evaluation.  With return_stats also returns an OccupancyStats."""
    if keep not in KEEP_RULES:
        raise ValueError(f"occupancy_mask: keep must be one of {sorted(KEEP_RULES)}, got {keep!r}")
    if device is None:
        device = next((t.device for t in (alphas, rgb) if torch.is_tensor(t) and t.device.type == "cuda"), "cuda:0")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.PixieHipError("occupancy_mask runs on a HIP device only (no CPU fallback)")
    a, c = _as_device_array(alphas, dev, "alphas"), _as_device_array(rgb, dev, "rgb")
    if c.dim() != 4 or c.shape[3] != 3:
        raise ValueError(f"occupancy_mask: rgb must be (D, H, W, 3), got {tuple(c.shape)}")
    D, H, W = (int(s) for s in c.shape[:3])
    if tuple(a.shape) not in ((D, H, W), (D, H, W, 1)):
        raise ValueError(f"occupancy_mask: alphas must be {(D, H, W)} or {(D, H, W, 1)}, got {tuple(a.shape)}")
    if a.dtype != c.dtype:                                             # float16 widens exactly
        a, c = a.float(), c.float()
    a, c = a.contiguous(), c.contiguous()
    if axes is None:
        axes = reference_axes((D, H, W), voxel_size, min_bounds)
    if any(torch.is_tensor(x) and x.device.type != "cpu" for x in axes):
        raise ValueError("occupancy_mask: axes must be host arrays (their spacing is checked on the host, without a read-back)")
    host_axes = [torch.as_tensor(np.asarray(x), dtype=torch.float32).contiguous() for x in axes]
    if [len(x) for x in host_axes] != [D, H, W]:
        raise ValueError(f"occupancy_mask: axes of {[len(x) for x in host_axes]} points for a grid of {(D, H, W)}")
    spacing = _lattice_spacing(host_axes, voxel_size)
    dev_axes = [x.to(dev) for x in host_axes]

    lib = _lib.load()
    desc = OccupancyDesc()
    desc.d_alphas, desc.d_rgb = a.data_ptr(), c.data_ptr()
    desc.d_axis_x, desc.d_axis_y, desc.d_axis_z = (x.data_ptr() for x in dev_axes)
    desc.dtype = 0 if a.dtype == torch.float16 else 1
    desc.d, desc.h, desc.w = D, H, W
    desc.run_filters, desc.nb_neighbors, desc.min_points, desc.keep = int(bool(run_outlier_filter)), int(nb_neighbors), int(min_cluster_pts), KEEP_RULES[keep]
    desc.voxel_size, desc.lattice_spacing = float(voxel_size), spacing
    desc.alpha_threshold, desc.gray_threshold, desc.std_ratio, desc.eps_multiplier = float(alpha_threshold), float(gray_threshold), float(std_ratio), float(eps_multiplier)
    with torch.cuda.device(dev):
        want_mean_dist = bool(return_stats and run_outlier_filter)
        need = lib.pixie_occupancy_scratch_bytes(C.byref(desc), int(want_mean_dist))
        if need < 0:
            check(1, "pixie_occupancy_scratch_bytes", lib=lib)
        mask8 = torch.empty((D, H, W), dtype=torch.uint8, device=dev)
        counts = torch.empty(8, dtype=torch.int64, device=dev)
        stats = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
        mean_dist = torch.empty((D, H, W), dtype=torch.float64, device=dev) if want_mean_dist else None
        scratch = torch.empty(max(int(need), 16), dtype=torch.uint8, device=dev)
        desc.d_stats = stats.data_ptr()
        check(lib.pixie_occupancy_mask(C.byref(desc), C.c_void_p(mask8.data_ptr()), C.c_void_p(mean_dist.data_ptr() if mean_dist is not None else 0),
                                       C.c_void_p(counts.data_ptr()), C.c_void_p(scratch.data_ptr()), _lib.current_stream_ptr()),
              "pixie_occupancy_mask", lib=lib)
        # inputs and scratch go back to torch's caching allocator here; launches queued on this stream are ordered before any reuse
        mask = mask8.view(torch.bool)
    return (mask, OccupancyStats(counts, stats, mean_dist)) if return_stats else mask


def create_occupancy_mask(output_path: str, alphas, rgb, voxel_size: float, min_bounds: Sequence[float] = (-0.5,) * 3, device="cuda:0",
                          **mask_kwargs) -> str:
    """voxelize.py:188-263 for the arrays extract_clip_voxel_grid holds: writes the bool (D, H, W) mask to
    output_path.replace('.npz', '_mask.npy') and returns that path.  mask_kwargs: the keywords of occupancy_mask."""
    mask = occupancy_mask(alphas, rgb, voxel_size, min_bounds, device=device, **mask_kwargs)
    mask_path = output_path.replace(".npz", "_mask.npy")
    os.makedirs(os.path.dirname(os.path.abspath(mask_path)), exist_ok=True)
    np.save(mask_path, mask.cpu().numpy())
    return mask_path


def occupancy_points(feature_grid_path: str, alpha_threshold: float = 0.01, gray_threshold: float = 0.05, voxel_downsample_size: float = 0.01,
                     device="cuda:0"):
    """compute_occupancy_point_cloud (voxelize.py:266-406) without Open3D: (xyz (n, 3) float32, rgb (n, 3) float32, metrics), device
    tensors in C order of the grid and the reference's metric keys.  The coordinates are torch.linspace(min, max, n) per axis
    (:319-321); the filters are remove_statistical_outlier(50, 4.0) and remove_floating_clusters(min_points=10, eps = 5 *
    voxel_downsample_size), i.e. keep="largest".  Colours above 1 are divided by 255 (:383-384).

    voxel_down_sample is not restated: at a cell size no larger than the lattice spacing every cell holds at most one voxel, so it
    is the identity up to the order of the points.  A larger voxel_downsample_size would merge voxels and is refused.  The
    reference's assertion that the grid is 64^3 (:301) is not kept: any grid with one spacing works."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.PixieHipError("occupancy_points runs on a HIP device only (no CPU fallback)")
    meta = np.load(feature_grid_path)
    min_bounds, max_bounds = np.asarray(meta["min_bounds"], np.float64), np.asarray(meta["max_bounds"], np.float64)
    grid_shape = meta["grid_shape"]
    alphas = np.load(feature_grid_path.replace(".npz", "_alphas.npy"))
    rgb = np.load(feature_grid_path.replace(".npz", "_rgb.npy"))
    axes = [torch.linspace(float(min_bounds[a]), float(max_bounds[a]), int(grid_shape[a])) for a in range(3)]
    spacing = _lattice_spacing(axes, voxel_downsample_size)
    if voxel_downsample_size > spacing * (1.0 + 1e-6):
        raise ValueError(f"occupancy_points: voxel_downsample_size {voxel_downsample_size} exceeds the lattice spacing {spacing:.6g}; "
                         "merging voxels is not supported")
    mask, stats = occupancy_mask(alphas, rgb, voxel_downsample_size, alpha_threshold=alpha_threshold, gray_threshold=gray_threshold,
                                 nb_neighbors=50, std_ratio=4.0, min_cluster_pts=10, eps_multiplier=5.0, keep="largest", return_stats=True,
                                 axes=axes, device=dev)
    idx = torch.nonzero(mask)
    xyz = torch.stack([axes[a].to(dev)[idx[:, a]] for a in range(3)], dim=1)
    colours = torch.from_numpy(np.ascontiguousarray(rgb)).to(dev)[idx[:, 0], idx[:, 1], idx[:, 2]].float()
    if colours.numel() > 0 and float(colours.max()) > 1.0:
        colours = colours / 255.0
    c = stats.counts
    metric = {"grid_shape": grid_shape, "init_num_voxels": int(grid_shape[0]) * int(grid_shape[1]) * int(grid_shape[2]),
              "num_voxels_after_density_threshold": c["after_density"],
              "num_voxels_after_gray_background_filtering": c["after_gray"],
              "num_voxels_after_downsampling": c["after_gray"],
              "num_voxels_after_outlier_removal": c["after_outlier_removal"],
              "num_voxels_after_floating_cluster_removal": c["after_cluster_removal"],
              "final_num_voxels": c["after_cluster_removal"]}
    return xyz, colours, metric


def load_voxel_scene(npz_path: str, device="cuda:0", recompute_mask: bool = False, **mask_kwargs):
    """What neural_scene_rollout takes of a voxelised scene: (feat_grid (1, C, D, H, W) float32 via load_voxel_grid, mask (D, H, W)
    bool, min_bounds, max_bounds), all from the files extract_clip_voxel_grid leaves next to `npz_path`.  The mask is
    <stem>_mask.npy when that file exists and recompute_mask is false; otherwise it is computed from <stem>_alphas.npy and
    <stem>_rgb.npy with the metadata's voxel_size and min_bounds (mask_kwargs: the keywords of occupancy_mask)."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.PixieHipError("load_voxel_scene runs on a HIP device only (no CPU fallback)")
    meta = np.load(npz_path)
    min_bounds, max_bounds = tuple(float(v) for v in meta["min_bounds"]), tuple(float(v) for v in meta["max_bounds"])
    feat = load_voxel_grid(npz_path.replace(".npz", "_features.npy"), dev)
    mask_path = npz_path.replace(".npz", "_mask.npy")
    if os.path.exists(mask_path) and not recompute_mask:
        if mask_kwargs:
            raise ValueError("load_voxel_scene: mask keywords given, but the stored mask is used; pass recompute_mask=True")
        mask = torch.from_numpy(np.load(mask_path)).to(dev) > 0
    else:
        mask = occupancy_mask(np.load(npz_path.replace(".npz", "_alphas.npy")), np.load(npz_path.replace(".npz", "_rgb.npy")),
                              float(meta["voxel_size"]), min_bounds, device=dev, **mask_kwargs)
    return feat, mask, min_bounds, max_bounds
