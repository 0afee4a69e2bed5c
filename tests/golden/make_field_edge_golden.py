#!/usr/bin/env python
"""Writes tests/golden/field_edges.npz: the edges of the field -> particle transfer as the REFERENCE's own code computes them.

`unscale_prediction`, `get_mat_id` and `map_pred_to_ply` (pixie/voxel/map_pred_to_coords.py:41-75,122-126,128-283) are cut
out of the reference file with `ast` and executed UNMODIFIED, with the `plyfile` stand-in of make_mapping_golden.py (their
module imports hydra / plyfile, which are not installed here).  Two records:

  un_*    `unscale_prediction` on an (11, 4, 5, 6) tensor whose three continuous channels each hold values inside [-1, 1],
          exactly +-1, the float32 neighbours of +-1 on both sides, values beyond +-1, +-inf and NaN -- once per range set:
          the shipped normalization_ranges.yaml, pixie_amd.synthetic.PIPELINE_RANGES, and a set that no float32 represents
          (density 1.861 ... 4.154, E 3.04 ... 11.112, nu 0.2103 ... 0.4493), where float32(max - min) and
          float32(max) - float32(min) differ.
  one_*   `map_pred_to_ply` on a prediction with ONE class channel that stores the ids 0 ... 7 as floats: get_mat_id takes
          the channel as the class index, the confidence is 1.  The 12 x 10 x 9 scene sits in the corner of the 64^3 grid
          that map_pred_to_ply asserts (:182); the occupied corner and the vertex columns are kept.

Run in the build container (needs /root/reference); the .npz holds data only and is committed.  tests/test_field_oracle.py
pins oracle/field_oracle.py to it bit for bit, tests/test_field_edges_hip.py compares the kernels with it.
"""
import json
import logging
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_mapping_golden import REF, PlyData, PlyElement, cut  # noqa: E402
from pixie_amd.synthetic import PIPELINE_RANGES  # noqa: E402

RANGE_KEYS = ("density_min", "density_max", "E_min", "E_max", "nu_min", "nu_max")
ODD_RANGES = {"density_min": 1.861, "density_max": 4.154, "E_min": 3.04, "E_max": 11.112, "nu_min": 0.2103, "nu_max": 0.4493}
G = 64
CORNER = (12, 10, 9)


def edge_tensor(seed=5):
    rng = np.random.default_rng(seed)
    t = rng.normal(0, 0.6, size=(11, 4, 5, 6)).astype(np.float32)
    one = np.float32(1.0)
    special = np.array([1.0, -1.0, np.nextafter(one, np.float32(2)), np.nextafter(-one, np.float32(-2)), np.nextafter(one, np.float32(0)),
                        np.nextafter(-one, np.float32(0)), 1.5, -3.0, 1e30, -1e30, np.inf, -np.inf, np.nan, 0.0, -0.0], dtype=np.float32)
    for c in range(3):
        flat = t[c].reshape(-1)                                  # a view: different places in every channel
        flat[7 * c + 3 * np.arange(len(special))] = special
    assert all(np.isnan(t[c]).sum() == 1 and np.isinf(t[c]).sum() == 2 and (np.abs(t[c]) == 1).sum() == 2 for c in range(3))
    return t


def one_channel_scene(seed=23):
    rng = np.random.default_rng(seed)
    D, H, W = CORNER
    pred = np.zeros((4, D, H, W), np.float32)
    pred[:3] = rng.normal(0, 0.7, size=(3, D, H, W)).astype(np.float32)
    pred[3] = rng.integers(0, 8, size=(D, H, W)).astype(np.float32)
    mask = (rng.random((D, H, W)) < 0.6).astype(np.float32)
    lo = np.array([-0.6, -0.5, -0.7]); hi64 = np.array([2.1, 3.0, 2.9])      # bounds of the whole 64^3 grid
    return pred, mask, lo, hi64


def main():
    shipped = json.load(open(f"{REF}/normalization_stats/normalization_ranges.yaml"))
    sets = [shipped, dict(PIPELINE_RANGES), ODD_RANGES]
    ns = {"np": np, "os": os, "json": json, "Path": Path, "logging": logging, "PlyData": PlyData, "PlyElement": PlyElement,
          "DictConfig": object}
    exec(cut(f"{REF}/pixie/voxel/map_pred_to_coords.py", ["unscale_prediction", "get_mat_id", "transform_nerf_to_world", "map_pred_to_ply"]), ns)
    cfg_of = lambda r: types.SimpleNamespace(training=types.SimpleNamespace(**{k: float(r[k]) for k in RANGE_KEYS}))
    out = {"range_keys": np.array(RANGE_KEYS), "ranges": np.array([[float(r[k]) for k in RANGE_KEYS] for r in sets], np.float64)}

    t = edge_tensor()
    out["un_pred"] = t
    with np.errstate(all="ignore"):
        out["un_out"] = np.stack([ns["unscale_prediction"](t, cfg_of(r)) for r in sets])
    assert out["un_out"].dtype == np.float32 and all(np.isnan(out["un_out"][s, c]).sum() == 1 for s in range(3) for c in range(3))

    pred, mask, lo, hi64 = one_channel_scene()
    pad = lambda a: np.pad(a, [(0, 0)] * (a.ndim - 3) + [(0, G - n) for n in CORNER])
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "pred.npy"), pad(pred)); np.save(os.path.join(tmp, "mask.npy"), pad(mask))
        np.savez(os.path.join(tmp, "grid.npz"), min_bounds=lo, max_bounds=hi64, grid_shape=np.array([G, G, G]))
        ply = os.path.join(tmp, "out.ply")
        ns["map_pred_to_ply"](os.path.join(tmp, "pred.npy"), os.path.join(tmp, "mask.npy"), os.path.join(tmp, "grid.npz"), ply, "obj",
                              cfg=cfg_of(shipped))
        v = PlyData.read(ply)["vertex"].data
    assert len(v) == int(mask.sum()) and sorted(np.unique(v["material_id"])) == list(range(8))
    out.update(one_pred=pred, one_mask=mask, one_min_bounds=lo, one_max_bounds=hi64, one_grid=np.array([G, G, G]))
    for name in ("x", "y", "z", "part_label", "density", "E", "nu", "material_id", "conf"):
        out[f"one_ply_{name}"] = v[name]
    path = os.path.join(HERE, "field_edges.npz")
    np.savez_compressed(path, **out)
    print("wrote field_edges.npz:", os.path.getsize(path), "bytes;", len(v), "points;", {k: a.shape for k, a in out.items()})


if __name__ == "__main__":
    main()
