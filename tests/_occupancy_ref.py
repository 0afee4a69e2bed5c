"""NumPy / scipy restatement of the occupancy mask (pixie/voxel/voxelize.py:_create_occupancy_mask and the same filters of
compute_occupancy_point_cloud), the reference of tests/test_occupancy_*.py, and the scenes those tests run.  No torch.

Stage A   float32(alpha) > float32(alpha_threshold) and ((r + g) + b) / 3 > float32(gray_threshold), in float32: the order of
          torch's float32 mean over three channels (f3rm_robot/optimize.py:290-293).
Stage B   Open3D's RemoveStatisticalOutliers: m_i = mean distance to the k' = min(nb_neighbors, M) nearest candidates, the point
          itself included, by scipy.spatial.cKDTree.query(k=k') on the float64 values of the float32 coordinates; cloud_mean =
          sum m / M, std = sqrt(sum (m - cloud_mean)^2 / (M - 1)); keep m > 0 and m < cloud_mean + std_ratio std.
Stage C   Open3D's ClusterDBSCAN: neighbours are the pairs with ((dx dx + dy dy) + dz dz) < eps eps in float64, strict.  The pairs
          that the expression is evaluated on come from cKDTree.query_pairs with a radius a little above eps -- a superset of the
          ball, so the float64 expression alone decides membership -- in chunks.  Core: >= min_points in the open ball, itself
          included.  Clusters: components of the core points, numbered by ascending lowest core index (C order of the grid);
          border points take the lowest-numbered cluster with a core point in reach; the rest is -1.
Keep      "non_noise": label != -1 (voxelize.py:250).  "largest": the cluster with the most members, first maximum; everything if
          all is noise (optimize.py:44-89).
"""
import numpy as np

# scipy is imported inside the functions of the restatement: the scene builders below need numpy only

F32 = np.float32

DEFAULTS = dict(alpha_threshold=0.01, gray_threshold=0.05, nb_neighbors=50, std_ratio=4.0, min_cluster_pts=10, eps_multiplier=5.0)
OTHER = dict(alpha_threshold=0.01, gray_threshold=0.05, nb_neighbors=8, std_ratio=1.0, min_cluster_pts=4, eps_multiplier=2.5)
EDGE = dict(DEFAULTS, std_ratio=1000.0)          # the edge scenes: stage B keeps every candidate, stage C runs at its defaults
EPS_RULES = ("strict", "closed", "int_strict", "int_closed")


# ---------------------------------------------------------------- the restatement
def make_axes(shape, voxel_size, min_bounds=(-0.5, -0.5, -0.5)):
    """float32(min + i voxel_size), i < n: torch.arange(min, max, voxel_size) of f3rm_robot/initial_proposals.py:18-27 for the
    count the grid has"""
    return [(np.float64(lo) + np.arange(n, dtype=np.float64) * np.float64(voxel_size)).astype(F32) for n, lo in zip(shape, min_bounds)]


def lattice_deviation(axes):
    """E of the m_i bar: the largest float64 deviation of an axis coordinate from axis[0] + i (axis[-1] - axis[0]) / (n - 1)"""
    e = 0.0
    for a in axes:
        a = a.astype(np.float64)
        if len(a) > 1:
            e = max(e, float(np.max(np.abs(a - (a[0] + np.arange(len(a)) * (a[-1] - a[0]) / (len(a) - 1))))))
    return e


def classify(alphas, rgb, alpha_threshold, gray_threshold):
    a = np.asarray(alphas).reshape(np.asarray(rgb).shape[:3]).astype(F32)
    c = np.asarray(rgb).astype(F32)
    dense = a > F32(alpha_threshold)
    mean = ((c[..., 0] + c[..., 1]) + c[..., 2]) / F32(3.0)
    return dense, dense & (mean > F32(gray_threshold))


def coords_of(mask, axes):
    i, j, k = np.nonzero(mask)                                     # C order
    return np.stack([axes[0][i], axes[1][j], axes[2][k]], axis=1).astype(np.float64)


def stage_b(cand, axes, nb_neighbors, std_ratio):
    pts = coords_of(cand, axes)
    big_m = len(pts)
    out = dict(M=big_m, m=np.zeros(0), cloud_mean=np.nan, std=np.nan, threshold=np.nan, keep=np.zeros_like(cand))
    if big_m == 0:
        return out
    from scipy.spatial import cKDTree
    kp = min(nb_neighbors, big_m)
    dist, _ = cKDTree(pts).query(pts, k=kp)
    m = dist.reshape(big_m, kp).sum(axis=1) / kp
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = m.sum() / big_m
        std = np.sqrt(((m - mean) ** 2).sum() / np.float64(big_m - 1))
    thr = mean + std_ratio * std
    keep_pts = (m > 0) & (m < thr)
    keep = np.zeros_like(cand)
    keep[cand] = keep_pts
    out.update(m=m, cloud_mean=mean, std=std, threshold=thr, keep=keep)
    return out


def open_ball_pairs(pts, eps, chunk=1 << 20, rule="strict", idx=None, multiplier=None):
    """(a, b), a < b, of every pair inside the ball.  rule "strict" is the one under test: ((dx dx + dy dy) + dz dz) < eps eps in
    float64.  The others exist so that tests can show that a wrong rule changes the outcome: "closed" is <= in float64;
    "int_strict" / "int_closed" compare the integer squared index offset (idx: the points' voxel indices) with multiplier^2."""
    from scipy.spatial import cKDTree
    if len(pts) < 2:
        return np.zeros((0, 2), np.int64)
    cand = cKDTree(pts).query_pairs(eps * (1.0 + 1e-3), output_type="ndarray").astype(np.int64)
    keep = np.zeros(len(cand), bool)
    eps2 = np.float64(eps) * np.float64(eps)
    for s in range(0, len(cand), chunk):
        a, b = cand[s:s + chunk, 0], cand[s:s + chunk, 1]
        if rule in ("strict", "closed"):
            d = pts[b] - pts[a]
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            keep[s:s + chunk] = d2 < eps2 if rule == "strict" else d2 <= eps2
        else:
            n = ((idx[b] - idx[a]) ** 2).sum(axis=1)
            keep[s:s + chunk] = n < multiplier * multiplier if rule == "int_strict" else n <= multiplier * multiplier
    return cand[keep]


def dbscan_labels_open(pts, eps, min_points, **rule):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    n = len(pts)
    labels = np.full(n, -1, np.int64)
    if n == 0:
        return labels, 0
    pairs = open_ball_pairs(pts, eps, **rule)
    degree = np.ones(n, np.int64)                                  # the point itself
    np.add.at(degree, pairs[:, 0], 1)
    np.add.at(degree, pairs[:, 1], 1)
    core = degree >= min_points
    cc = pairs[core[pairs[:, 0]] & core[pairs[:, 1]]]
    ncomp, comp = connected_components(coo_matrix((np.ones(len(cc), np.int8), (cc[:, 0], cc[:, 1])), shape=(n, n)), directed=False)
    core_idx = np.nonzero(core)[0]
    if len(core_idx) == 0:
        return labels, 0
    lowest = np.full(ncomp, n, np.int64)
    np.minimum.at(lowest, comp[core_idx], core_idx)
    order = np.argsort(lowest[np.unique(comp[core_idx])])
    number = np.full(ncomp, -1, np.int64)
    number[np.unique(comp[core_idx])[order]] = np.arange(len(order))
    labels[core_idx] = number[comp[core_idx]]
    best = np.full(n, np.iinfo(np.int64).max, np.int64)
    for a, b in ((0, 1), (1, 0)):                                  # border points: the lowest-numbered cluster in reach
        sel = core[pairs[:, a]] & ~core[pairs[:, b]]
        np.minimum.at(best, pairs[sel, b], labels[pairs[sel, a]])
    border = ~core & (best != np.iinfo(np.int64).max)
    labels[border] = best[border]
    return labels, len(order)


def keep_rule(labels, keep):
    if keep == "non_noise":
        return labels != -1
    if len(labels) == 0 or labels.max() < 0:
        return np.ones(len(labels), bool)
    return labels == np.argmax(np.bincount(labels[labels >= 0]))


def reference(scene, run_outlier_filter=True, eps_rule="strict", **params):
    """every intermediate of the mask of `scene` under DEFAULTS overridden by params; eps_rule other than "strict" is a WRONG rule
    (see open_ball_pairs), for tests that show the difference"""
    p = dict(DEFAULTS, **params)
    axes = scene["axes"]
    dense, cand = classify(scene["alphas"], scene["rgb"], p["alpha_threshold"], p["gray_threshold"])
    out = dict(dense=dense, cand=cand, n_density=int(dense.sum()), n_gray=int(cand.sum()))
    if not run_outlier_filter:
        return out
    b = stage_b(cand, axes, p["nb_neighbors"], p["std_ratio"])
    out.update(m=b["m"], cloud_mean=b["cloud_mean"], std=b["std"], threshold=b["threshold"], stage_b=b["keep"], n_stage_b=int(b["keep"].sum()))
    eps = float(scene["voxel_size"]) * float(p["eps_multiplier"])
    labels, n_clusters = dbscan_labels_open(coords_of(b["keep"], axes), eps, p["min_cluster_pts"], rule=eps_rule,
                                            idx=np.stack(np.nonzero(b["keep"]), axis=1), multiplier=float(p["eps_multiplier"]))
    out.update(labels=labels, n_clusters=n_clusters, eps=eps)
    for rule in ("non_noise", "largest"):
        mask = np.zeros_like(cand)
        mask[b["keep"]] = keep_rule(labels, rule)
        out[rule] = mask
    return out


def exact_eps_pairs(mask, axes, eps, multiplier):
    """(inside, outside): lattice pairs of `mask` at exactly `multiplier` voxels (integer squared offset == multiplier^2) on either
    side of the strict float64 comparison"""
    idx = np.stack(np.nonzero(mask), axis=1)
    pts = coords_of(mask, axes)
    if len(pts) < 2:
        return 0, 0
    from scipy.spatial import cKDTree
    pairs = cKDTree(pts).query_pairs(eps * (1.0 + 1e-3), output_type="ndarray")
    di = idx[pairs[:, 1]] - idx[pairs[:, 0]]
    at_eps = (di * di).sum(axis=1) == int(round(multiplier * multiplier))
    d = pts[pairs[at_eps, 1]] - pts[pairs[at_eps, 0]]
    inside = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) < np.float64(eps) * np.float64(eps)
    return int(inside.sum()), int((~inside).sum())


# ---------------------------------------------------------------- scenes
SHAPES = {"tiny16": ((16, 16, 16), 1.0 / 16), "inexact24": ((24, 24, 24), 1.0 / 24), "slab": ((20, 12, 33), 1.0 / 33),
          "word70": ((9, 11, 70), 1.0 / 70), "scene64": ((64, 64, 64), 1.0 / 64)}
EXTRA_SHAPES = {"scene128": ((128, 128, 128), 1.0 / 128)}          # scripts/profile_occupancy.py only: no test runs it
_cache = {}


def build_scene(name, seed=0):
    """an ellipsoid body, a one-voxel-thick plate, about 40 stray single voxels, one detached clump of 12 voxels and 5 % dark
    voxels; alphas (D, H, W, 1) and rgb (D, H, W, 3) float16, as voxelize.py writes them"""
    key = (name, seed)
    if key in _cache:
        return _cache[key]
    shape, voxel_size = SHAPES[name] if name in SHAPES else EXTRA_SHAPES[name]
    rng = np.random.default_rng(1000 + seed + sum(map(ord, name)))
    dims = np.array(shape)
    ii, jj, kk = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    centre, radii = dims * 0.45, np.maximum(dims * 0.24, 2.0)
    occ = (((ii - centre[0]) / radii[0]) ** 2 + ((jj - centre[1]) / radii[1]) ** 2 + ((kk - centre[2]) / radii[2]) ** 2) <= 1.0
    plate_i = min(int(centre[0] + radii[0]) + 3, shape[0] - 1)
    occ |= (ii == plate_i) & (jj >= shape[1] // 8) & (jj < shape[1] - shape[1] // 8) & (kk >= shape[2] // 8) & (kk < shape[2] - shape[2] // 8)
    occ |= (ii < 2) & (jj >= shape[1] - 2) & (kk >= shape[2] - 3)                  # the clump: 2 x 2 x 3 in a corner
    free = np.nonzero(~occ.reshape(-1))[0]
    occ.reshape(-1)[rng.choice(free, size=40, replace=False)] = True
    alphas = rng.uniform(0.0, 0.005, shape)
    alphas[occ] = rng.uniform(0.3, 1.0, int(occ.sum()))
    rgb = rng.uniform(0.2, 0.9, shape + (3,))
    dark = occ & (rng.uniform(size=shape) < 0.05)
    rgb[dark] = rng.uniform(0.0, 0.03, (int(dark.sum()), 3))
    scene = dict(name=name, shape=shape, voxel_size=voxel_size, min_bounds=(-0.5, -0.5, -0.5), axes=make_axes(shape, voxel_size),
                 alphas=alphas.astype(np.float16)[..., None], rgb=rgb.astype(np.float16))
    _cache[key] = scene
    return scene


def few_scene(count):
    """16^3 with `count` candidates (7, 2, 1 or 0): k' = M and the degenerate statistics"""
    shape, voxel_size = (16, 16, 16), 1.0 / 16
    spots = [(3, 4, 5), (3, 4, 6), (3, 5, 5), (4, 4, 5), (9, 9, 9), (12, 2, 14), (0, 15, 0)][:count]
    alphas = np.zeros(shape + (1,), np.float16)
    rgb = np.full(shape + (3,), 0.5, np.float16)
    for s in spots:
        alphas[s] = 0.8
    return dict(name=f"few{count}", shape=shape, voxel_size=voxel_size, min_bounds=(-0.5, -0.5, -0.5), axes=make_axes(shape, voxel_size),
                alphas=alphas, rgb=rgb)


EDGE_SHAPE = (60, 30, 70)
EDGE_SPACING = {"edge32": 1.0 / 32, "edge33": 1.0 / 33}            # a power-of-two lattice and an inexact one


def edge_scene(name):
    """Structures whose stage-C outcome is decided by lattice pairs at EXACTLY eps = 5 voxels (run with EDGE: stage B keeps all):
      dumbbells   two 2 x 2 x 3 blocks (12 voxels each, so every voxel is core) whose facing sides are 5 voxels apart: 24 along the
                  first axis at every start 0 .. 23, 16 along the last (bit-packed) axis, four of them across the 64-bit word
                  boundary.  Only offsets (5, 0, 0) / (0, 0, 5) bridge the blocks: one cluster if such a pair is inside, two if not.
      plates      28 times a 3 x 3 x 1 plate (9 voxels) and one voxel 5 voxels above its centre: the centre voxel's ball holds 10
                  iff that pair is inside, and then all ten voxels are a cluster; otherwise all ten are noise.
    On the power-of-two lattice every such pair is outside the open ball; on the 1/33 lattice float64 rounding decides pair by pair.
    Blocks of equal size also tie the `largest` rule.  The arrays are float32 with values no float16 holds, next to the thresholds:
    structure voxels sit one to three float32 steps above them, and a third of the other voxels are decoys at or just below one."""
    if name in _cache:
        return _cache[name]
    shape, voxel_size = EDGE_SHAPE, EDGE_SPACING[name]
    occ = np.zeros(shape, bool)
    lanes = (0, 9, 18, 27)
    n = 0
    for j0 in lanes:                                               # dumbbells along the first axis, i in [0, 33]
        for k0 in (0, 12, 24, 36, 48, 60):
            a = n % 24
            n += 1
            for i0 in (a, a + 6):
                occ[i0:i0 + 2, j0:j0 + 2, k0:k0 + 3] = True
    for lane, j0 in enumerate(lanes):                              # dumbbells along the last axis, i in [41, 42]
        for base in (0, 17, 34, 56):
            c = base + lane
            occ[41:43, j0:j0 + 2, c:c + 3] = True
            occ[41:43, j0:j0 + 2, c + 7:c + 10] = True
    n = 0
    for j0 in lanes:                                               # plates, i in [49, 59]
        for k0 in (0, 10, 20, 30, 40, 50, 60):
            pi = 49 + n % 6
            n += 1
            occ[pi, j0:j0 + 3, k0:k0 + 3] = True
            occ[pi + 5, j0 + 1, k0 + 1] = True
    rng = np.random.default_rng(77)
    at, gt = F32(DEFAULTS["alpha_threshold"]), F32(DEFAULTS["gray_threshold"])
    up = lambda v, steps: [v := np.nextafter(v, F32(np.inf), dtype=F32) for _ in range(steps)][-1]
    alphas = rng.uniform(0.0, 0.005, shape).astype(F32)
    rgb = rng.uniform(0.2, 0.9, shape + (3,)).astype(F32)
    steps = rng.integers(1, 4, shape)
    for st in (1, 2, 3):                                           # structure: alpha 1 .. 3 float32 steps above its threshold
        alphas[occ & (steps == st)] = up(at, st)
    above = F32(0.0500001)                                         # ((t + t) + t) / 3 in float32 must come out above gray_threshold
    assert ((above + above) + above) / F32(3.0) > gt
    rgb[occ & (steps == 2)] = above
    kind = rng.integers(0, 9, shape)
    alphas[~occ & (kind == 0)] = at                                # decoys: alpha == threshold (not above), bright
    alphas[~occ & (kind == 1)] = np.nextafter(at, F32(0.0), dtype=F32)
    grey = ~occ & (kind == 2)                                      # decoys: dense, mean colour at or below the threshold
    alphas[grey] = F32(0.7)
    below = gt
    while ((below + below) + below) / F32(3.0) > gt:
        below = np.nextafter(below, F32(0.0), dtype=F32)
    rgb[grey] = below
    scene = dict(name=name, shape=shape, voxel_size=voxel_size, min_bounds=(-0.5, -0.5, -0.5), axes=make_axes(shape, voxel_size),
                 alphas=alphas[..., None], rgb=rgb, structure=occ)
    _cache[name] = scene
    return scene


def all_scenes():
    return [build_scene(n) for n in SHAPES] + [few_scene(c) for c in (7, 2, 1, 0)] + [edge_scene(n) for n in EDGE_SPACING]
