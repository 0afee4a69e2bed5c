"""Shared by the GPU parity tests of the field -> particle transfer (tests/test_field_hip.py, tests/test_field_edges_hip.py):
the suite's bars, and the rule by which a particle may be left out of a comparison.

Bars: integer outputs (material id, part label) and the too-far set exact; float32 outputs within 2e-6 relative (powf and the
float64 defaults differ from numpy in the last ulp); distances within 1e-6."""
import numpy as np

REL_BAR, DIST_BAR = 2e-6, 1e-6
FLOAT_KEYS = ("density", "E", "nu", "conf")


def compare(got, ref, too_far, keep=None, equal_nan=False, worst=None):
    """`got`: the product's outputs as numpy arrays (+ n_too_far); `ref`: the oracle's; `too_far`: the oracle's too-far set.
    `keep`: boolean mask of the particles that are compared (default: all) -- n_too_far is then compared over all particles only
    if nobody is left out.  `equal_nan`: a NaN in the reference must be a NaN in the product, and nowhere else.
    `worst`: a dict that receives the worst relative error per float key and the worst distance error, each BEFORE it is
    asserted (so that a caller can report the figure of a failing comparison); it is also returned."""
    sel = np.ones(len(ref["material_id"]), bool) if keep is None else np.asarray(keep, bool)
    if sel.all():
        assert int(got["n_too_far"]) == int(too_far.sum())
    else:   # the particles left out may fall on either side of the threshold
        assert int(too_far[sel].sum()) <= int(got["n_too_far"]) <= int(too_far[sel].sum()) + int((~sel).sum())
    for key in ("material_id", "part_labels"):
        assert np.array_equal(got[key][sel], ref[key][sel]), key
    worst = {} if worst is None else worst
    for key in FLOAT_KEYS:
        g, r = got[key][sel].astype(np.float64), np.asarray(ref[key])[sel].astype(np.float64)
        if equal_nan:
            nan = np.isnan(r)
            assert np.array_equal(np.isnan(g), nan), key
            g, r = g[~nan], r[~nan]
        rel = np.abs(g - r) / np.maximum(np.abs(r), 1e-30)
        worst[key] = float(rel.max()) if rel.size else 0.0
        assert worst[key] < REL_BAR, (key, worst[key])
    worst["nearest_dist"] = float(np.abs(got["nearest_dist"][sel] - ref["nearest_dist"][sel]).max()) if sel.any() else 0.0
    assert worst["nearest_dist"] < DIST_BAR
    return worst


def cloud_distances(cloud_pos, particle_pos, k):
    """The k + 1 smallest particle -> material point distances, ascending, by brute force in float64 on the float32 coordinates
    (n, min(k + 1, number of points))."""
    d = np.linalg.norm(particle_pos.astype(np.float64)[:, None, :] - cloud_pos.astype(np.float64)[None, :, :], axis=2)
    return np.sort(d, axis=1)[:, :k + 1]


def borderline(cloud_pos, particle_pos, k, threshold):
    """Particles whose outcome the last bits of a distance decide, judged on the reference's side alone, in float64:
    rule 1: the nearest distance lies within 1e-6 of the too-far threshold;
    rule 2: the (k + 1)-th neighbour is as near as the k-th to 1e-6 relative: d_{k+1} - d_k <= 1e-6 d_k."""
    d = cloud_distances(cloud_pos, particle_pos, k)
    out = np.abs(d[:, 0] - threshold) <= 1e-6
    if d.shape[1] > k:
        out |= (d[:, k] - d[:, k - 1]) <= 1e-6 * d[:, k - 1]
    return out
