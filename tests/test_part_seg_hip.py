"""GPU checks of the part segmentation (pixie_amd.part_segmentation, pixie_amd/csrc/part_segmentation.hip) against the float64
restatement of tests/_part_seg_ref.py.

Bars.  Stage A: labels equal the restatement wherever its top-two margin exceeds tau = 2 C 2^-24 (tests/test_part_seg_ref.py asserts
that at most 1 % of every scene lies inside, so the exclusion cannot hide a failure); counts equal a bincount of the labels; the
material grid is EQUAL to a NumPy fill; |score - float64 score| <= C 2^-24 / (2 T) + 8 2^-24 on every voxel.  Stage B: every masked
voxel equals the restatement under the (squared offset, C index) rule; nothing is excluded.  Two runs are bit-identical.

The score distances are printed here; profiles/part_segmentation_parity.txt is written from the same scenes and the same restatement
by scripts/part_seg_bench.py --parity (a test run leaves the tree as it found it).
"""
import os

import numpy as np
import pytest
import torch

from tests import _part_seg_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_refs, _votes = {}, {}


def scene_of(name):
    return R.duplicate_scene() if name == "duplicate" else R.stage_a_scene(name)


def ref_of(name, temperature=0.1):
    """computed once per scene, shared and left unchanged"""
    if (name, temperature) not in _refs:
        sc = scene_of(name)
        _refs[(name, temperature)] = (sc, R.stage_a64(sc["features"], sc["mask"], sc["queries"], temperature))
    return _refs[(name, temperature)]


def vote_ref(name, parts, k):
    if (name, parts, k) not in _votes:
        grid = R.vote_scene(name, parts)
        _votes[(name, parts, k)] = (grid, R.vote(grid, k)["voted"])
    return _votes[(name, parts, k)]


def run(sc, **kw):
    from pixie_amd.part_segmentation import part_segmentation
    return part_segmentation(torch.from_numpy(sc["features"]).to(DEV), torch.from_numpy(sc["mask"]).to(DEV), sc["queries"], **kw)


def check_stage_a(sc, ref, seg, temperature=0.1):
    mask, channels, parts = sc["mask"], sc["features"].shape[-1], len(sc["queries"])
    labels, scores = seg.label_grid.cpu().numpy(), seg.score_grid.cpu().numpy()
    assert labels.dtype == np.int8 and scores.dtype == np.float32 and labels.shape == mask.shape and seg.label_grid.is_cuda
    assert np.all(labels[~mask] == -1) and np.all(np.isnan(scores[~mask]))
    got, got_scores = labels[mask].astype(np.int64), scores[mask].astype(np.float64)
    clear = ref["margin"] > R.tau(channels)
    fine = ~np.isnan(ref["scores"])
    err = np.abs(got_scores[fine] - ref["scores"][fine])
    bar = R.score_bar(channels, temperature)
    print(f"{sc['name']}: {len(got)} voxels, {int((ref['margin'] <= R.tau(channels)).sum())} inside tau, "
          f"worst |score - ref| {err.max() if len(err) else 0.0:.3e}, bar {bar:.3e}")
    assert np.array_equal(got[clear], ref["labels"][clear]), "labels outside tau"
    assert got.min(initial=0) >= 0 and got.max(initial=0) < parts
    assert seg.counts == np.bincount(got, minlength=parts).tolist() and seg.n_masked == int(mask.sum())
    assert np.array_equal(np.isnan(got_scores), ~fine)
    assert np.all(err <= bar), f"scores: worst {err.max():.3e} against {bar:.3e}"
    # the lazy views are the mask's C order
    assert seg.part_labels.dtype == torch.int64 and np.array_equal(seg.part_labels.cpu().numpy(), got)
    assert np.array_equal(seg.part_scores.cpu().numpy(), scores[mask], equal_nan=True)
    return labels


@pytest.mark.parametrize("name", list(R.STAGE_A))
def test_stage_a_equals_the_restatement(name):
    """12 x 10 x 9 at C = 768, K = 5; C = 40, K = 1; C = 768, K = 32; C = 2048, K = 8; an empty and a full mask; one zero-norm row;
    `big`: 42 x 41 x 40 at C = 16 with about 41 k masked voxels, where a wave of ps_row_kernel walks several rows (its grid is 6144
    waves) and ps_count_kernel takes a second round (65 536 voxels per round).  The queries are float32, contiguous and not
    normalised"""
    from pixie_amd.part_segmentation import material_grid
    sc, ref = ref_of(name)
    seg = run(sc, props=sc["props"], background_id=7)
    labels = check_stage_a(sc, ref, seg)
    want = R.material_fill(labels, sc["props"], 7)
    assert np.array_equal(seg.material_grid.cpu().numpy(), want), "fused material grid"
    assert np.array_equal(material_grid(seg, sc["props"], background_id=3).cpu().numpy(), R.material_fill(labels, sc["props"], 3))
    assert seg.smoothed_grid is None and seg.slow_path_voxels == 0
    if name == "zero_row":
        assert labels[sc["mask"]][3] == 0 and np.isnan(seg.part_scores.cpu().numpy()[3])
    if name == "empty":
        assert seg.part_labels.numel() == 0 and seg.counts == [0, 0, 0]
    if name == "big":
        assert sc["mask"].size > 65536 and seg.n_masked > 4 * 6144


def test_duplicate_query_rows_tie_to_the_lower_index():
    sc = R.duplicate_scene()
    seg = run(sc)
    uniq = R.stage_a64(sc["features"], sc["mask"], sc["queries"][[0, 1, 3]])
    got = seg.part_labels.cpu().numpy()
    assert not np.any(got == 2) and np.any(got == 1) and seg.counts[2] == 0
    clear = uniq["margin"] > R.tau(128)
    assert np.array_equal(got[clear], np.array([0, 1, 3])[uniq["labels"]][clear])


def test_another_temperature_and_tensor_queries():
    sc, ref = ref_of("c768k5", 0.5)
    seg = run(dict(sc, queries=torch.from_numpy(sc["queries"]).to(DEV)), softmax_temperature=0.5)
    check_stage_a(sc, ref, seg, temperature=0.5)


@pytest.mark.parametrize("parts,k", [(2, 200), (6, 200), (6, 7), (2, 10)])
@pytest.mark.parametrize("name", R.VOTE_SCENES)
def test_vote_equals_the_restatement_on_every_voxel(name, parts, k):
    """24^3: a ball of radius 8, a one-voxel-thick plate (the slow path) and a ball with distant strays"""
    grid, want = vote_ref(name, parts, k)
    features, mask, queries = R.one_hot_inputs(grid, parts)
    props = np.arange(4 * parts, dtype=np.float32).reshape(parts, 4) + 1
    seg = run({"features": features, "mask": mask, "queries": queries}, smooth_k=k, props=props,
              axes=[np.linspace(-0.5, 0.5, 24, dtype=np.float32)] * 3)
    assert np.array_equal(seg.label_grid.cpu().numpy(), grid), "the one-hot inputs give the scene's labels exactly"
    voted = seg.smoothed_grid.cpu().numpy()
    print(f"{name} K={parts} k={k}: {int(mask.sum())} voxels, slow path {seg.slow_path_voxels}, {int((voted != grid).sum())} labels changed")
    assert voted.dtype == np.int8 and np.array_equal(voted, want)
    if name != "ball" and k == 200:
        assert seg.slow_path_voxels > 0, "the scene is there to run the cube bisection"
    assert np.array_equal(seg.material_grid.cpu().numpy(), R.material_fill(want, props, 7)), "filled from the voted labels"
    assert np.array_equal(seg.part_labels.cpu().numpy(), want[mask])
    assert seg.counts == np.bincount(grid[mask], minlength=parts).tolist(), "the counts stay stage A's"
    assert np.all(seg.part_scores.cpu().numpy() > 0.99), "the scores stay stage A's"


def test_slow_list_longer_than_the_slow_kernels_grid():
    """4900 plate voxels, all on the slow path at k = 100: the 4096 waves of ps_vote_slow_kernel stride, a wave votes for two voxels"""
    if "big_plate" not in _votes:
        grid = R.big_plate_scene()
        _votes["big_plate"] = (grid, R.vote(grid, 100)["voted"])
    grid, want = _votes["big_plate"]
    features, mask, queries = R.one_hot_inputs(grid, 6)
    seg = run({"features": features, "mask": mask, "queries": queries}, smooth_k=100)
    assert np.array_equal(seg.label_grid.cpu().numpy(), grid)
    assert seg.slow_path_voxels == int(mask.sum()) == 4900 > 4096
    assert np.array_equal(seg.smoothed_grid.cpu().numpy(), want)


def test_fewer_masked_voxels_than_k_raises_value_error():
    grid = np.full((6, 6, 6), -1, np.int8)
    grid[1:4, 1:4, 1:4] = 0
    features, mask, queries = R.one_hot_inputs(grid, 2)
    with pytest.raises(ValueError, match="fewer"):
        run({"features": features, "mask": mask, "queries": queries}, smooth_k=28)
    assert run({"features": features, "mask": mask, "queries": queries}, smooth_k=27).smoothed_grid[2, 2, 2].item() == 0


def test_refusals():
    from pixie_amd._lib import PixieHipError
    from pixie_amd.part_segmentation import part_segmentation
    f = torch.zeros((4, 4, 4, 16), dtype=torch.float16, device=DEV)
    m = torch.ones((4, 4, 4), dtype=torch.bool, device=DEV)
    q = np.ones((3, 16), np.float32)
    with pytest.raises(ValueError, match="smooth_k"):
        part_segmentation(f, m, q, smooth_k=256)
    with pytest.raises(ValueError, match="parts"):
        part_segmentation(f, m, np.ones((33, 16), np.float32))
    with pytest.raises(ValueError, match="multiple of 8"):
        part_segmentation(torch.zeros((4, 4, 4, 12), dtype=torch.float16, device=DEV), m, np.ones((3, 12), np.float32))
    with pytest.raises(ValueError, match="bytes of queries"):
        part_segmentation(torch.zeros((2, 2, 2, 2048), dtype=torch.float16, device=DEV), m[:2, :2, :2], np.ones((16, 2048), np.float32))
    with pytest.raises(ValueError, match="float16"):
        part_segmentation(f.float(), m, q)
    with pytest.raises(ValueError, match="float32"):
        part_segmentation(f, m, q.astype(np.float64))
    with pytest.raises(PixieHipError, match="HIP device"):
        part_segmentation(f.cpu(), m, q)
    with pytest.raises(PixieHipError, match="HIP device"):
        part_segmentation(f, m.cpu(), q)
    even = np.arange(4, dtype=np.float32)
    with pytest.raises(ValueError, match="one spacing"):
        part_segmentation(f, m, q, smooth_k=7, axes=[np.array([0.0, 1.0, 2.0, 4.0], np.float32)] * 3)
    with pytest.raises(ValueError, match="one spacing"):
        part_segmentation(f, m, q, smooth_k=7, axes=[even, even, 2 * even])
    with pytest.raises(ValueError, match="one spacing"):
        part_segmentation(f, m, q, smooth_k=7, axes=[even, even, -even])
    assert part_segmentation(f, m, q, smooth_k=7, axes=[0.25 * even] * 3).smoothed_grid is not None


def test_two_runs_are_bit_identical():
    sc, _ = ref_of("c768k5")
    grid, _ = vote_ref("strays", 6, 200)
    features, mask, queries = R.one_hot_inputs(grid, 6)
    props = np.arange(24, dtype=np.float32).reshape(6, 4)
    for inputs, kw in ((sc, dict(props=sc["props"])), ({"features": features, "mask": mask, "queries": queries}, dict(props=props, smooth_k=200))):
        a, b = run(inputs, **kw), run(inputs, **kw)
        assert torch.equal(a.label_grid, b.label_grid) and torch.equal(a.score_grid.view(torch.int32), b.score_grid.view(torch.int32))
        assert torch.equal(a.material_grid.view(torch.int32), b.material_grid.view(torch.int32)) and a.counts == b.counts
        if a.smoothed_grid is not None:
            assert torch.equal(a.smoothed_grid, b.smoothed_grid)


@pytest.mark.parametrize("smooth", [False, True])
def test_segment_scene_writes_the_reference_files(tmp_path, smooth):
    """the PLY round-trips through read_ply with the listed properties and dtypes, load_material_points reads it, and the grids
    equal a NumPy fill; the device is needed for the labels only"""
    from pixie_amd.field_mapping import load_material_points
    from pixie_amd.part_segmentation import TAB10, VERTEX_DTYPE, segment_scene
    from pixie_amd.ply_io import read_ply
    grid = R.vote_scene("ball", 6)
    features, mask, queries = R.one_hot_inputs(grid, 6)
    stem = str(tmp_path / "clip_features")
    lo, hi = np.array([-0.5, -0.4, -0.3]), np.array([0.5, 0.6, 0.7])
    np.savez(stem + ".npz", min_bounds=lo, max_bounds=hi, grid_shape=np.array(grid.shape))
    np.save(stem + "_features.npy", features)
    np.save(stem + "_mask.npy", mask)
    names = ["pot", "soil", "stem", "leaves", "petals", "rim"]
    material_props = {"material_dict": {n: {"density": 100.0 * (i + 1), "E": 1e5 * (i + 1), "nu": 0.1 + 0.05 * i, "material_id": i % 3} for i, n in enumerate(names)}}
    del material_props["material_dict"]["stem"]["E"], material_props["material_dict"]["rim"]["material_id"]     # the defaults of :334-337
    out = str(tmp_path / "out")
    n = int(mask.sum())
    rgb = np.random.default_rng(0).random((n, 3)).astype(np.float32)
    asked = []
    if smooth:
        metrics = segment_scene(stem + ".npz", material_props, queries, output_dir=out, use_spatial_smoothing=True, rgb=rgb)
    else:
        metrics = segment_scene(stem + ".npz", material_props, encode=lambda part_names: asked.append(list(part_names)) or queries, output_dir=out)
        assert asked == [names]
    want = vote_ref("ball", 6, 200)[1] if smooth else grid
    labels = want[mask].astype(np.int64)
    props = np.array([[100, 1e5, 0.1, 0], [200, 2e5, 0.15, 1], [300, 2e6, 0.2, 2], [400, 4e5, 0.25, 0], [500, 5e5, 0.3, 1], [600, 6e5, 0.35, 0]], np.float32)
    assert metrics["initial"] == 24 ** 3 and metrics["masked_voxels"] == n and metrics["num_parts"] == 6
    assert [metrics[f"part_{i}_{name}"] for i, name in enumerate(names)] == np.bincount(grid[mask], minlength=6).tolist()
    saved = np.load(os.path.join(out, "part_labels.npy"))
    assert saved.dtype == np.int64 and np.array_equal(saved, labels)
    fill = R.material_fill(want, props, 7)
    assert np.array_equal(np.load(os.path.join(out, "material_grid.npy")), fill)
    for channel, fname in enumerate(("density_grid.npy", "E_grid.npy", "nu_grid.npy", "material_id_grid.npy")):
        assert np.array_equal(np.load(os.path.join(out, fname)), fill[..., channel])
    axes = [torch.linspace(float(lo[a]), float(hi[a]), 24).numpy() for a in range(3)]
    idx = np.argwhere(mask)
    for fname in ("segmented_semantics.ply", "segmented_rgb.ply"):
        vertex, _ = read_ply(os.path.join(out, fname))
        assert [(name, vertex.dtype[name].str[1:]) for name in vertex.dtype.names] == VERTEX_DTYPE and len(vertex) == n
        for a, key in enumerate("xyz"):
            assert np.allclose(vertex[key], axes[a][idx[:, a]], rtol=0, atol=1e-6)
        assert np.array_equal(vertex["part_label"], labels) and np.array_equal(vertex["material_id"], props[labels, 3].astype(np.int32))
        for column, key in enumerate(("density", "E", "nu")):
            assert np.array_equal(vertex[key], props[labels, column])
        assert np.all(vertex["alpha"] == 255)
        if fname == "segmented_semantics.ply":
            tab = (np.array(TAB10, np.float32) * 255).astype(np.uint8)
            assert tab[0].tolist() == [(np.float32(c / 255.0) * 255).astype(np.uint8) for c in (31, 119, 180)]
            assert np.array_equal(np.stack([vertex["red"], vertex["green"], vertex["blue"]], axis=1), tab[labels])
        else:
            want_rgb = (rgb * 255).astype(np.uint8) if smooth else np.full((n, 3), 255, np.uint8)
            assert np.array_equal(np.stack([vertex["red"], vertex["green"], vertex["blue"]], axis=1), want_rgb)
    points = load_material_points(os.path.join(out, "segmented_semantics.ply"), device=DEV)
    assert tuple(points["pos"].shape) == (n, 3) and np.array_equal(points["part_labels"], labels)
    assert np.array_equal(points["E"], props[labels, 1]) and np.array_equal(points["material_id"], props[labels, 3].astype(np.int32))
