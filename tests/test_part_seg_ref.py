"""CPU checks of the restatement the part-segmentation tests compare against (tests/_part_seg_ref.py), so that what the GPU tests
exclude cannot hide a failure.

Stage A.  The reference's own float32 torch expression agrees with the float64 restatement on every label whose float64 top-two
margin exceeds tau = 2 C 2^-24, and on every scene the tests use at most 1 % of the masked voxels lie inside tau.
Stage B.  The vote under the (squared offset, C index) rule equals sklearn's KDTree.query(k) + scipy.stats.mode -- the reference's
local_post_process_segmentation -- on every voxel whose vote is decided (top count - second count > 2 m, m = min(t, S - t) for t
members taken from a last shell of S), at least 80 % of the voxels of each vote scene are decided, and with k = 7 (the last shell
taken whole, m = 0) every voxel agrees.
"""
import numpy as np
import pytest

from tests import _part_seg_ref as R

STAGE_A_SCENES = [n for n in R.STAGE_A if n != "empty"]


def scene_of(name):
    return R.duplicate_scene() if name == "duplicate" else R.stage_a_scene(name)


@pytest.mark.parametrize("name", STAGE_A_SCENES)
def test_float32_torch_agrees_with_float64_outside_tau(name):
    sc = scene_of(name)
    ref = R.stage_a64(sc["features"], sc["mask"], sc["queries"])
    labels, scores = R.stage_a_torch(sc["features"], sc["mask"], sc["queries"])
    channels = sc["features"].shape[-1]
    clear = ref["margin"] > R.tau(channels)
    inside = int((ref["margin"] <= R.tau(channels)).sum())              # a zero row has no margin: it is checked on its own
    err = np.abs(scores[clear].astype(np.float64) - ref["scores"][clear])
    print(f"{name}: {len(labels)} voxels, {inside} inside tau {R.tau(channels):.2e}, smallest margin {np.nanmin(ref['margin']):.3e}, "
          f"worst |score32 - score64| {err.max():.3e} (bar {R.score_bar(channels):.3e})")
    assert np.array_equal(labels[clear], ref["labels"][clear])
    assert inside <= 0.01 * len(labels)
    assert np.all(err <= R.score_bar(channels))


def test_duplicate_queries_leave_the_tie_to_the_unique_rows():
    """with row 2 a copy of row 1 the margin is 0 wherever they win; judged on the unique rows (0, 1, 3) at most 1 % lie inside tau"""
    sc = R.duplicate_scene()
    ref = R.stage_a64(sc["features"], sc["mask"], sc["queries"])
    uniq = R.stage_a64(sc["features"], sc["mask"], sc["queries"][[0, 1, 3]])
    assert not np.any(ref["labels"] == 2) and np.any(ref["labels"] == 1)
    assert np.array_equal(np.array([0, 1, 3])[uniq["labels"]], ref["labels"])
    assert int((uniq["margin"] <= R.tau(128)).sum()) <= 0.01 * len(ref["labels"])


def test_zero_row_is_label_0_and_score_nan_in_both():
    sc = R.stage_a_scene("zero_row")
    ref = R.stage_a64(sc["features"], sc["mask"], sc["queries"])
    labels, scores = R.stage_a_torch(sc["features"], sc["mask"], sc["queries"])
    assert ref["labels"][3] == 0 and np.isnan(ref["scores"][3]) and labels[3] == 0 and np.isnan(scores[3])
    assert np.isnan(ref["scores"]).sum() == 1


_votes = {}


def vote_of(name, parts, k):
    if (name, parts, k) not in _votes:
        _votes[(name, parts, k)] = R.vote(R.vote_scene(name, parts), k)
    return _votes[(name, parts, k)]


def tree_vote(label_grid, k):
    neighbors = pytest.importorskip("sklearn.neighbors")
    stats = pytest.importorskip("scipy.stats")
    import torch
    axes = [torch.linspace(-0.5, 0.5, s).numpy() for s in label_grid.shape]
    idx = np.argwhere(label_grid >= 0)
    coords = np.stack([axes[a][idx[:, a]] for a in range(3)], axis=1)
    labs = label_grid[label_grid >= 0].astype(np.int64)
    _, nearest = neighbors.KDTree(coords).query(coords, k=k)
    return stats.mode(labs[nearest], axis=1, keepdims=False).mode


@pytest.mark.parametrize("name,parts,k", [("ball", 2, 200), ("ball", 6, 200), ("ball", 2, 10), ("plate", 6, 200), ("plate", 2, 200), ("strays", 2, 200),
                                          ("strays", 2, 10)])
def test_vote_equals_the_kd_tree_where_decided(name, parts, k):
    grid = R.vote_scene(name, parts)
    v = vote_of(name, parts, k)
    ok = R.decided(v)
    print(f"{name} K={parts} k={k}: {len(ok)} voxels, {ok.mean():.1%} decided")
    assert ok.mean() >= 0.8
    tree = tree_vote(grid, k)
    ours = v["voted"][grid >= 0]
    assert np.array_equal(ours[ok], tree[ok])


@pytest.mark.parametrize("name", ["ball", "strays"])
def test_k7_takes_the_last_shell_whole_and_every_voxel_agrees(name):
    grid = R.vote_scene(name, 6)
    v = vote_of(name, 6, 7)
    interior = v["taken"] == v["shell"]                                    # m = 0: the neighbour sets are the same, ties included
    assert interior.mean() > 0.7, "k = 7 is one voxel and its six face neighbours wherever they are all masked"
    tree = tree_vote(grid, 7)
    ours = v["voted"][grid >= 0]
    assert np.array_equal(ours[interior], tree[interior])
    assert np.array_equal(ours[R.decided(v)], tree[R.decided(v)])


def test_material_fill_and_vote_shapes():
    grid = R.vote_scene("ball", 2)
    props = np.arange(8, dtype=np.float32).reshape(2, 4)
    m = R.material_fill(grid, props, background_id=7)
    assert m.shape == grid.shape + (4,) and np.array_equal(m[grid < 0], np.tile([0, 0, 0, 7], ((grid < 0).sum(), 1)))
    assert np.array_equal(m[grid == 1], np.tile(props[1], ((grid == 1).sum(), 1)))
