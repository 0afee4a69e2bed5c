#!/usr/bin/env python
"""Writes tests/golden/occupancy_mask.npz: the occupancy mask of the 64^3 scene of tests/_occupancy_ref.py (the grid size the
reference insists on, pixie/voxel/voxelize.py:301) as the NumPy / scipy restatement in that file computes it, under both parameter
sets the tests run (DEFAULTS: extract_clip_voxel_grid's; OTHER: nb_neighbors 8, std_ratio 1, eps_multiplier 2.5, min_cluster_pts 4).

Per parameter set `p`: {p}_cand, {p}_stage_b, {p}_non_noise, {p}_largest (np.packbits of the C-order masks), {p}_m (float64, the
candidates only, C order), {p}_counts (after density, after gray, after stage B, after stage C, clusters) and {p}_stats (cloud_mean,
std, threshold).  `build(scene)` returns the same dict without touching the file; tests/test_occupancy_ref.py checks that the
committed file reproduces from it.  Needs numpy and scipy only.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _occupancy_ref as R  # noqa: E402

OUT = os.path.join(HERE, "occupancy_mask.npz")
PARAM_SETS = {"defaults": R.DEFAULTS, "other": R.OTHER}


def build(scene=None):
    scene = scene or R.build_scene("scene64")
    out = {"shape": np.array(scene["shape"], np.int64)}
    for p, params in PARAM_SETS.items():
        r = R.reference(scene, **params)
        for k in ("cand", "stage_b", "non_noise", "largest"):
            out[f"{p}_{k}"] = np.packbits(r[k].reshape(-1))
        out[f"{p}_m"] = r["m"].astype(np.float64)
        out[f"{p}_counts"] = np.array([r["n_density"], r["n_gray"], r["n_stage_b"], int(r["non_noise"].sum()), r["n_clusters"]], np.int64)
        out[f"{p}_stats"] = np.array([r["cloud_mean"], r["std"], r["threshold"]], np.float64)
    return out


def unpack(golden, p, shape):
    """the record of parameter set p in the shape reference() returns"""
    n = int(np.prod(shape))
    r = {k: np.unpackbits(golden[f"{p}_{k}"])[:n].reshape(shape).astype(bool) for k in ("cand", "stage_b", "non_noise", "largest")}
    c = golden[f"{p}_counts"]
    r.update(m=golden[f"{p}_m"], n_density=int(c[0]), n_gray=int(c[1]), n_stage_b=int(c[2]), n_clusters=int(c[4]),
             cloud_mean=float(golden[f"{p}_stats"][0]), std=float(golden[f"{p}_stats"][1]), threshold=float(golden[f"{p}_stats"][2]))
    return r


if __name__ == "__main__":
    np.savez_compressed(OUT, **build())
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
