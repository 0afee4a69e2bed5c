"""Restatement of pixie/voxel/segmentation.py for the tests of the part segmentation.

    stage_a64()       run_clip + clip_part_segmentation (:98-168) in float64 NumPy: the reference for labels and scores
    stage_a_torch()   the reference's own lines (:77-80, 103-120, 164-168) as float32 torch-CPU expressions
    vote()            local_post_process_segmentation (:190-226) under the project's last-shell rule: neighbours ordered by (integer
                      squared offset, C-order linear index), the first k taken, equal counts to the smallest label
    material_fill()   the grid of :429-452 as NumPy masks
    scenes            stage-A scenes are fp16(a q_label + noise) with margins near 0.1; vote scenes are piecewise-constant label
                      regions with salt noise on a 24^3 grid

tau(C) = 2 C 2^-24: a float32 dot of unit vectors of length C is off by at most C 2^-24, and the top-two margin compares two of them.
score_bar(C, T) = C 2^-24 / (2 T) + 8 2^-24: sum_j |d score / d sim_j| <= 1 / (2 T), and 8 2^-24 covers expf and the division.
"""
import numpy as np

EPS = 2.0 ** -24


def tau(channels):
    return 2.0 * channels * EPS


def score_bar(channels, temperature=0.1):
    return channels * EPS / (2.0 * temperature) + 8.0 * EPS


def stage_a64(features, mask, queries, temperature=0.1):
    """features (D, H, W, C) float16, mask (D, H, W) bool, queries (K, C) -> dict over the masked voxels in C order: labels, scores,
    margin (top sim minus the second, inf for K = 1, NaN for a zero row), and the dense label / score grids."""
    f = features.reshape(-1, features.shape[-1])[mask.reshape(-1)].astype(np.float64)
    q = np.asarray(queries, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = f / np.linalg.norm(f, axis=-1, keepdims=True)
        q = q / np.linalg.norm(q, axis=-1, keepdims=True)
        sims = f @ q.T
        labels = np.argmax(sims, axis=1) if len(sims) else np.zeros(0, np.int64)     # NaN rows: 0, as torch.argmax
        top = np.take_along_axis(sims, labels[:, None], axis=1)[:, 0] if len(sims) else np.zeros(0)
        scores = 1.0 / np.exp((sims - top[:, None]) / temperature).sum(axis=1)
        if sims.shape[1] > 1:
            rest = sims.copy()
            rest[np.arange(len(rest)), labels] = -np.inf
            margin = top - rest.max(axis=1)
        else:
            margin = np.where(np.isnan(top), np.nan, np.inf)
    label_grid = np.full(mask.shape, -1, np.int8)
    label_grid[mask] = labels
    score_grid = np.full(mask.shape, np.nan, np.float64)
    score_grid[mask] = scores
    return {"labels": labels, "scores": scores, "margin": margin, "sims": sims, "label_grid": label_grid, "score_grid": score_grid}


def stage_a_torch(features, mask, queries, temperature=0.1):
    """the reference's lines on the CPU in float32: (part_labels int64, part_scores float32) over the masked voxels in C order"""
    import torch
    features_tensor = torch.from_numpy(features)
    features_flat = features_tensor.reshape(-1, features_tensor.shape[-1])
    linear_mask = torch.from_numpy(mask.reshape(-1))
    features_filtered = features_flat[linear_mask]
    features_filtered = features_filtered.to(torch.float32)
    features_filtered /= features_filtered.norm(dim=-1, keepdim=True)
    query_embs = torch.from_numpy(np.ascontiguousarray(queries, np.float32)).float().clone()
    query_embs /= query_embs.norm(dim=-1, keepdim=True)
    similarities = features_filtered @ query_embs.T
    scaled_similarities = similarities / temperature
    probabilities = torch.nn.functional.softmax(scaled_similarities, dim=1)
    part_labels = torch.argmax(probabilities, dim=1)
    part_scores = torch.gather(probabilities, 1, part_labels.unsqueeze(1)).squeeze(1)
    return part_labels.numpy(), part_scores.numpy()


def vote(label_grid, k):
    """label_grid (D, H, W) int, -1 outside the mask -> dict: voted (D, H, W) int8, and per masked voxel in C order: taken (members
    taken from the last shell), shell (masked members of the last shell), lead (top count minus the second count)."""
    d, h, w = label_grid.shape
    idx = np.flatnonzero(label_grid.reshape(-1) >= 0)
    labs = label_grid.reshape(-1)[idx].astype(np.int64)
    n = len(idx)
    assert n >= k
    ijk = np.stack(np.unravel_index(idx, (d, h, w)), axis=1).astype(np.int64)
    n_labels = int(labs.max()) + 1
    voted = np.full(label_grid.shape, -1, np.int8)
    taken, shell, lead = (np.zeros(n, np.int64) for _ in range(3))
    for a in range(n):
        off = ((ijk - ijk[a]) ** 2).sum(axis=1)
        order = np.argsort(off * (d * h * w) + idx, kind="stable")[:k]         # (squared offset, C index), both exact integers
        counts = np.bincount(labs[order], minlength=max(n_labels, 2))
        voted.reshape(-1)[idx[a]] = np.argmax(counts)                          # first maximum: the smallest label
        last = off[order[-1]]
        taken[a] = int((off[order] == last).sum())
        shell[a] = int((off == last).sum())
        top2 = np.sort(counts)[-2:]
        lead[a] = top2[1] - top2[0]
    return {"voted": voted, "taken": taken, "shell": shell, "lead": lead, "index": idx}


def decided(v):
    """top count - second count > 2 m, m = min(t, S - t): exchanging m members of the last shell moves a count difference by <= 2 m"""
    m = np.minimum(v["taken"], v["shell"] - v["taken"])
    return v["lead"] > 2 * m


def material_fill(label_grid, props, background_id=7):
    grid = np.zeros(label_grid.shape + (4,), np.float32)
    grid[..., 3] = background_id
    on = label_grid >= 0
    grid[on] = np.asarray(props, np.float32)[label_grid[on]]
    return grid


# ---------------------------------------------------------------- stage-A scenes
STAGE_A = {   # name: (shape, C, K, mask rule)
    "c768k5": ((12, 10, 9), 768, 5, "blob"),
    "c40k1": ((6, 5, 7), 40, 1, "blob"),
    "c768k32": ((7, 6, 5), 768, 32, "blob"),
    "c2048k8": ((6, 5, 5), 2048, 8, "blob"),
    "empty": ((5, 4, 6), 64, 3, "empty"),
    "full": ((5, 6, 7), 64, 3, "full"),
    "zero_row": ((6, 5, 4), 128, 4, "blob"),
    # 68 880 voxels, about 41 k masked: more than the 6144 waves of the row kernel's grid (a wave walks several rows, the next row's
    # loads in flight) and more than the 65 536 voxels one round of the count kernel's grid covers
    "big": ((42, 41, 40), 16, 5, "blob"),
}


def stage_a_scene(name, seed=0):
    """features = fp16(scale (a q_label / |q_label| + noise)) with |noise| ~ 1 and a = 0.1 sqrt(...) chosen so that the winning
    similarity is near 0.1 above the rest; the queries are float32, contiguous and NOT normalised."""
    shape, channels, parts, rule = STAGE_A[name]
    rng = np.random.default_rng([seed, channels, parts])
    queries = (rng.standard_normal((parts, channels)) * rng.uniform(0.5, 4.0, (parts, 1))).astype(np.float32)
    unit = queries.astype(np.float64) / np.linalg.norm(queries.astype(np.float64), axis=1, keepdims=True)
    want = rng.integers(0, parts, shape)
    noise = rng.standard_normal(shape + (channels,)) / np.sqrt(channels)
    features = (2.5 * (0.14 * unit[want] + noise)).astype(np.float16)
    if rule == "empty":
        mask = np.zeros(shape, bool)
    elif rule == "full":
        mask = np.ones(shape, bool)
    else:
        mask = rng.random(shape) < 0.6
    if name == "zero_row":
        i, j, k = np.argwhere(mask)[3]
        features[i, j, k] = 0
    props = np.stack([rng.uniform(100, 2000, parts), rng.uniform(1e4, 1e7, parts), rng.uniform(0.1, 0.45, parts),
                      rng.integers(0, 7, parts)], axis=1).astype(np.float32)
    return {"name": name, "shape": shape, "features": features, "mask": mask, "queries": np.ascontiguousarray(queries), "props": props}


def duplicate_scene():
    """K = 4 with query row 2 a copy of row 1: every voxel that prefers them sees a tie, which goes to index 1"""
    sc = stage_a_scene("zero_row", seed=5)
    i, j, k = np.argwhere(sc["mask"])[3]
    sc["features"][i, j, k] = sc["features"][i, j, (k + 1) % sc["shape"][2]]
    sc["queries"][2] = sc["queries"][1]
    sc["name"] = "duplicate"
    return sc


# ---------------------------------------------------------------- vote scenes
VOTE_SHAPE = (24, 24, 24)
VOTE_SCENES = ("ball", "plate", "strays")


def vote_scene(name, parts, seed=0):
    """(label_grid (24, 24, 24) int8 with -1 outside the mask): piecewise-constant regions with 4 % salt noise"""
    rng = np.random.default_rng([seed, parts, VOTE_SCENES.index(name)])
    i, j, k = np.meshgrid(*(np.arange(s) for s in VOTE_SHAPE), indexing="ij")
    r2 = (i - 12) ** 2 + (j - 11) ** 2 + (k - 12) ** 2
    if name == "ball":
        mask = r2 <= 64
    elif name == "plate":
        mask = (i == 9) & (j >= 2) & (j < 22) & (k >= 1) & (k < 23)
    else:
        mask = (r2 <= 64) | (rng.random(VOTE_SHAPE) < 0.0015)
    if parts == 2:
        region = (j + k // 3 >= 15).astype(np.int64)
    else:
        region = ((j >= 11).astype(np.int64) + 2 * (k >= 8).astype(np.int64) + 2 * (k >= 16).astype(np.int64)) % parts
    salt = rng.random(VOTE_SHAPE) < 0.04
    labels = np.where(salt, rng.integers(0, parts, VOTE_SHAPE), region)
    return np.where(mask, labels, -1).astype(np.int8)


def big_plate_scene(parts=6, seed=0):
    """a one-voxel-thick 70 x 70 plate in a (3, 72, 72) grid: 4900 voxels that all leave the fast path at k > 81 (a plane holds 81
    offsets with n <= 25), more than the 4096 waves of the slow kernel's grid, so a wave takes a second voxel"""
    rng = np.random.default_rng([seed, parts, 99])
    shape = (3, 72, 72)
    i, j, k = np.meshgrid(*(np.arange(s) for s in shape), indexing="ij")
    mask = (i == 1) & (j >= 1) & (j < 71) & (k >= 1) & (k < 71)
    region = ((j >= 36).astype(np.int64) + 2 * (k >= 24).astype(np.int64) + 2 * (k >= 48).astype(np.int64)) % parts
    labels = np.where(rng.random(shape) < 0.04, rng.integers(0, parts, shape), region)
    return np.where(mask, labels, -1).astype(np.int8)


def one_hot_inputs(label_grid, parts, channels=8):
    """features and queries whose stage-A labels are exactly label_grid's: q_j = (j + 1) e_j, f = e_label (sim 1 against 0)"""
    queries = np.zeros((parts, channels), np.float32)
    queries[np.arange(parts), np.arange(parts)] = np.arange(1, parts + 1)
    features = np.zeros(label_grid.shape + (channels,), np.float16)
    on = label_grid >= 0
    features[on, label_grid[on]] = 1.0
    return features, on, queries
