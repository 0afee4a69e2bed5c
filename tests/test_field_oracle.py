"""oracle/field_oracle.py against the golden vectors produced by the reference's own code
(tests/golden/make_field_golden.py executes unscale_prediction / MaterialProperties cut out of the reference files)."""
import os

import numpy as np
import pytest

from oracle import field_oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden", "field_transfer.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_unscale_and_point_cloud_match_reference(gold):
    un = field_oracle.unscale_prediction(gold["pred"])
    assert np.array_equal(un, gold["unscaled"])
    cloud = field_oracle.voxel_point_cloud(un, gold["mask"], gold["min_bounds"], gold["max_bounds"])
    for key in ("pos", "density", "E", "nu", "material_id", "part_labels", "conf"):
        assert cloud[key].dtype == gold["cloud_" + key].dtype
        assert np.array_equal(cloud[key], gold["cloud_" + key]), key


@pytest.mark.parametrize("weighted", [False, True])
def test_knn_assignment_matches_reference(gold, weighted):
    out = field_oracle.field_to_particles(gold["pred"], gold["mask"], gold["min_bounds"], gold["max_bounds"], gold["particle_pos"],
                                          k=10, nn_distance_threshold=0.1, weighted=weighted)
    tag = "w_" if weighted else "u_"
    assert out["too_far"].sum() == gold[tag + "too_far"].sum() > 0
    for key in ("part_labels", "density", "E", "nu", "material_id", "conf", "nearest_dist", "too_far"):
        assert np.array_equal(out[key], gold[tag + key]), key
    far = out["too_far"]
    assert (out["material_id"][far] == field_oracle.STATIONARY_ID).all() and (out["part_labels"][far] == 0).all()


EDGES = os.path.join(os.path.dirname(__file__), "golden", "field_edges.npz")


@pytest.fixture(scope="module")
def edges():
    return np.load(EDGES)


def edge_ranges(edges, s):
    return {str(k): float(v) for k, v in zip(edges["range_keys"], edges["ranges"][s])}


@pytest.mark.parametrize("s", [0, 1, 2])
def test_unscale_edges_match_reference(edges, s):
    """tests/golden/make_field_edge_golden.py: +-1, their float32 neighbours, values beyond, +-inf and NaN in every continuous
    channel, for the shipped ranges, PIPELINE_RANGES and a set that is not exact in float32 -- bit for bit, NaN where the
    reference has NaN."""
    from pixie_amd.synthetic import PIPELINE_RANGES
    r = edge_ranges(edges, s)
    assert r == [field_oracle.NORMALIZATION_RANGES, PIPELINE_RANGES, r][s]
    pred, want = edges["un_pred"], edges["un_out"][s]
    with np.errstate(all="ignore"):
        un = field_oracle.unscale_prediction(pred, r)
    assert un.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert nan[:3].sum() == 3 and np.array_equal(nan[:3], np.isnan(pred[:3])) and not nan[3:].any()
    assert np.array_equal(np.isnan(un), nan) and np.array_equal(un[~nan], want[~nan])
    assert np.isfinite(un[:3][np.isinf(pred[:3])]).all()                       # +-inf clip to the ends of the range


def test_single_class_channel_point_cloud_matches_reference(edges):
    """map_pred_to_ply on a (3 + 1)-channel prediction: get_mat_id (map_pred_to_coords.py:122-126) takes the one class channel
    as the class index; conf = 1."""
    G = tuple(int(n) for n in edges["one_grid"])
    pad = lambda a: np.pad(a, [(0, 0)] * (a.ndim - 3) + [(0, g - n) for g, n in zip(G, a.shape[-3:])])
    pred, mask = pad(edges["one_pred"]), pad(edges["one_mask"])
    cloud = field_oracle.voxel_point_cloud(field_oracle.unscale_prediction(pred), mask, edges["one_min_bounds"], edges["one_max_bounds"])
    assert np.array_equal(cloud["pos"], np.stack([edges["one_ply_x"], edges["one_ply_y"], edges["one_ply_z"]], 1))
    for key, col in (("density", "density"), ("E", "E"), ("nu", "nu"), ("conf", "conf"), ("material_id", "material_id"),
                     ("part_labels", "part_label")):
        assert cloud[key].dtype == edges["one_ply_" + col].dtype and np.array_equal(cloud[key], edges["one_ply_" + col]), key
    assert sorted(np.unique(cloud["material_id"])) == list(range(8)) and (cloud["conf"] == 1.0).all()
    assert np.array_equal(cloud["material_id"], edges["one_pred"][3][edges["one_mask"] > 0].astype(np.int32))


@pytest.mark.parametrize("weighted", [False, True])
def test_single_class_channel_ids_reach_the_particles(edges, weighted):
    """field_to_particles with one class channel: every particle's id is the mode (weighted: the heaviest id) of the CHANNEL'S
    VALUES at its K nearest occupied voxels, worked out here by brute force -- not 0, which argmax over one channel gives."""
    pred, mask = edges["one_pred"], edges["one_mask"]
    D, H, W = mask.shape
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([1.1, 0.9, 0.8])
    rng = np.random.default_rng(3)
    pos = (lo + (hi - lo) * rng.random((400, 3))).astype(np.float32)
    k = 5
    out = field_oracle.field_to_particles(pred, mask, lo, hi, pos, k=k, nn_distance_threshold=0.5, weighted=weighted)
    assert not out["too_far"].any()
    g = np.stack(np.meshgrid(np.linspace(lo[0], hi[0], D), np.linspace(lo[1], hi[1], H), np.linspace(lo[2], hi[2], W), indexing="ij"), -1)
    pts = g[mask > 0].astype(np.float32).astype(np.float64)
    ids = pred[3][mask > 0].astype(np.int32)
    d = np.linalg.norm(pos.astype(np.float64)[:, None, :] - pts[None], axis=2)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    want = np.empty(len(pos), np.int32)
    for i, nb in enumerate(order):
        w = 1.0 / (d[i, nb] + 1e-8) if weighted else np.ones(k)
        votes = np.bincount(ids[nb], weights=w, minlength=8)
        best = np.flatnonzero(votes == votes.max())
        want[i] = best[0] if weighted else next(j for j in ids[nb] if j in best)     # np.argmax / Counter.most_common(1)
    assert np.array_equal(out["material_id"], want) and np.array_equal(out["part_labels"], want)
    assert len(np.unique(want)) == 8 and (out["conf"] == 1.0).all()
