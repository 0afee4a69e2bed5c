"""GPU checks of the occupancy mask (pixie_amd.occupancy, pixie_amd/csrc/occupancy.hip) against the NumPy / scipy restatement of
tests/_occupancy_ref.py -- for the 64^3 scene against tests/golden/occupancy_mask.npz, which that restatement wrote.

Bars.  Every voxel of every scene is compared; nothing is excluded (tests/test_occupancy_ref.py shows that no candidate lies within
100 bars of the stage-B threshold).  The candidate bitmap, the stage-B mask, the stage-C mask under both keep rules, every count and
the cluster count are EQUAL.  |m_i - ref| <= 4 E + 1e-12 with E the largest float64 deviation of an axis coordinate from the uniform
lattice through the axis' end points (derived in tests/test_occupancy_math.py; 0 on the exact lattices).

The stage-B mask is observed, not recomputed: with min_cluster_pts = 1 every survivor is a core voxel, so the call's mask IS the
stage-B mask.  The candidate bitmap likewise is the mask of run_outlier_filter=False.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import _occupancy_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = {"defaults": R.DEFAULTS, "other": R.OTHER, "edge": R.EDGE}
SCENES = list(R.SHAPES) + ["few7", "few2", "few1", "few0"]
_refs = {}


def scene_of(name):
    return R.few_scene(int(name[3:])) if name.startswith("few") else R.edge_scene(name) if name in R.EDGE_SPACING else R.build_scene(name)


def ref_of(name, p):
    """computed once per (scene, parameter set), shared and left unchanged; scene64 comes from the golden file"""
    if (name, p) not in _refs:
        if name == "scene64":
            spec = importlib.util.spec_from_file_location("make_occupancy_golden", os.path.join(HERE, "golden", "make_occupancy_golden.py"))
            mk = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mk)
            with np.load(os.path.join(HERE, "golden", "occupancy_mask.npz")) as g:
                _refs[(name, p)] = mk.unpack(g, p, tuple(int(v) for v in g["shape"]))
        else:
            _refs[(name, p)] = R.reference(scene_of(name), **PARAMS[p])
    return _refs[(name, p)]


def run(scene, dtype=np.float16, squeeze=False, **kw):
    from pixie_amd.occupancy import occupancy_mask
    alphas = scene["alphas"].astype(dtype)
    if squeeze:
        alphas = alphas[..., 0]
    return occupancy_mask(alphas, scene["rgb"].astype(dtype), scene["voxel_size"], scene["min_bounds"], axes=scene["axes"], **kw)


def check_all(scene, ref, params, dtype=np.float16, squeeze=False):
    bar = 4.0 * R.lattice_deviation(scene["axes"]) + 1e-12
    mask, stats = run(scene, dtype, squeeze, return_stats=True, **params)
    largest = run(scene, dtype, squeeze, keep="largest", **params)
    stage_b = run(scene, dtype, squeeze, **dict(params, min_cluster_pts=1))
    cand = run(scene, dtype, squeeze, run_outlier_filter=False, **params)
    assert mask.dtype == torch.bool and tuple(mask.shape) == scene["shape"] and mask.is_cuda
    m = stats.mean_dist.cpu().numpy()
    counts = stats.counts
    err = np.abs(m[ref["cand"]] - ref["m"])
    print(f"{scene['name']}: M {ref['n_gray']}, slow path {counts['slow_path_voxels']}, worst |m - ref| {err.max() if len(err) else 0.0:.3e}, bar {bar:.3e}, "
          f"clusters {counts['n_clusters']}")
    assert np.array_equal(cand.cpu().numpy(), ref["cand"]), "candidate bitmap"
    assert np.array_equal(~np.isnan(m), ref["cand"]), "m is NaN exactly off the candidates"
    assert np.all(err <= bar), f"m: worst {err.max():.3e} against {bar:.3e}"
    assert np.array_equal(stage_b.cpu().numpy(), ref["stage_b"]), "stage-B mask"
    assert np.array_equal(mask.cpu().numpy(), ref["non_noise"]), "stage-C mask, non_noise"
    assert np.array_equal(largest.cpu().numpy(), ref["largest"]), "stage-C mask, largest"
    assert [counts[k] for k in ("after_density", "after_gray", "after_outlier_removal", "after_cluster_removal")] == \
        [ref["n_density"], ref["n_gray"], ref["n_stage_b"], int(ref["non_noise"].sum())]
    assert counts["n_clusters"] == ref["n_clusters"]
    if ref["n_gray"] > 2:
        assert [stats.cloud_mean, stats.std, stats.threshold] == pytest.approx([ref["cloud_mean"], ref["std"], ref["threshold"]], rel=1e-12, abs=bar)
    return stats


@pytest.mark.parametrize("name", list(R.EDGE_SPACING))
def test_edge_scenes_where_pairs_at_exactly_eps_decide(name):
    """Dumbbells bridged only by a 5-voxel pair and plates whose centre is core only through one: the expected masks change under a
    closed ball or an integer-offset comparison (tests/test_occupancy_ref.py::test_the_eps_rule_decides_the_edge_scenes), on a
    power-of-two and on a 1/33 lattice.  float32 inputs that no float16 holds, one step either side of both thresholds; clusters of
    equal size tie the `largest` rule."""
    scene, ref = scene_of(name), ref_of(name, "edge")
    stats = check_all(scene, ref, R.EDGE, dtype=np.float32)
    assert np.array_equal(ref["cand"], scene["structure"])
    assert stats.counts["n_clusters"] == ref["n_clusters"] >= 80
    assert 0 < int(ref["largest"].sum()) < int(ref["non_noise"].sum())


def test_mixed_dtypes_are_widened():
    """float16 alphas with float32 colours (and the reverse): the float16 array widens exactly"""
    from pixie_amd.occupancy import occupancy_mask
    scene, ref = scene_of("slab"), ref_of("slab", "defaults")
    for da, dc in ((np.float16, np.float32), (np.float32, np.float16)):
        mask = occupancy_mask(scene["alphas"].astype(da), scene["rgb"].astype(dc), scene["voxel_size"], scene["min_bounds"], axes=scene["axes"])
        assert np.array_equal(mask.cpu().numpy(), ref["non_noise"])


@pytest.mark.parametrize("p", ["defaults", "other"])
@pytest.mark.parametrize("name", SCENES)
def test_mask_equals_the_restatement(name, p):
    stats = check_all(scene_of(name), ref_of(name, p), PARAMS[p])
    if name == "tiny16" and p == "defaults":
        assert stats.counts["slow_path_voxels"] > 0.5 * stats.counts["after_gray"]
    if name == "few2":
        assert stats.std == 0.0 and stats.counts["after_outlier_removal"] == 0
    if name == "few1":
        assert np.isnan(stats.std) and stats.counts["after_outlier_removal"] == 0
    if name == "few0":
        assert stats.counts["after_gray"] == 0 and stats.counts["after_cluster_removal"] == 0


@pytest.mark.parametrize("name", ["slab", "word70", "few7"])
def test_float32_inputs_and_a_squeezed_alpha(name):
    check_all(scene_of(name), ref_of(name, "defaults"), R.DEFAULTS, dtype=np.float32, squeeze=True)


def test_two_calls_are_bit_equal():
    scene = scene_of("inexact24")
    a, sa = run(scene, return_stats=True)
    b, sb = run(scene, return_stats=True)
    assert torch.equal(a, b)
    assert torch.equal(sa.mean_dist.view(torch.int64), sb.mean_dist.view(torch.int64))
    assert sa.counts == sb.counts and [sa.cloud_mean, sa.std, sa.threshold] == [sb.cloud_mean, sb.std, sb.threshold]


def test_side_stream_with_the_default_stream_busy():
    scene, ref = scene_of("slab"), ref_of("slab", "defaults")
    busy = torch.randn(2048, 2048, device="cuda")
    side = torch.cuda.Stream()
    for _ in range(8):
        busy = busy @ busy * 1e-3                                      # queued on the default stream, not waited for
    with torch.cuda.stream(side):
        mask, stats = run(scene, return_stats=True)
    side.synchronize()
    assert np.array_equal(mask.cpu().numpy(), ref["non_noise"])
    assert stats.counts["after_outlier_removal"] == ref["n_stage_b"]
    torch.cuda.synchronize()


def write_scene_files(tmp_path, scene, features=4):
    path = str(tmp_path / "clip_features.npz")
    max_bounds = tuple(lo + n * scene["voxel_size"] for lo, n in zip(scene["min_bounds"], scene["shape"]))
    np.savez_compressed(path, min_bounds=scene["min_bounds"], max_bounds=max_bounds, voxel_size=scene["voxel_size"], feature_dim=features,
                        grid_shape=scene["shape"])
    feats = np.random.default_rng(3).standard_normal(scene["shape"] + (features,)).astype(np.float16)
    np.save(path.replace(".npz", "_features.npy"), feats)
    np.save(path.replace(".npz", "_alphas.npy"), scene["alphas"])
    np.save(path.replace(".npz", "_rgb.npy"), scene["rgb"])
    return path, feats, max_bounds


def test_file_round_trip(tmp_path):
    from pixie_amd.occupancy import create_occupancy_mask, load_voxel_scene
    scene, ref = scene_of("inexact24"), ref_of("inexact24", "defaults")
    path, feats, max_bounds = write_scene_files(tmp_path, scene)
    # no _mask.npy yet: computed from the alphas and colours
    feat, mask, lo, hi = load_voxel_scene(path, "cuda:0")
    assert np.array_equal(mask.cpu().numpy(), ref["non_noise"]) and mask.dtype == torch.bool
    assert tuple(feat.shape) == (1, 4) + scene["shape"] and feat.dtype == torch.float32
    assert np.array_equal(feat[0].permute(1, 2, 3, 0).cpu().numpy(), feats.astype(np.float32))
    assert lo == pytest.approx(scene["min_bounds"]) and hi == pytest.approx(max_bounds)
    # the file create_occupancy_mask writes: name, dtype and shape of voxelize.py:256-262
    mask_path = create_occupancy_mask(path, scene["alphas"], scene["rgb"], scene["voxel_size"], scene["min_bounds"])
    assert mask_path == path.replace(".npz", "_mask.npy")
    stored = np.load(mask_path)
    assert stored.dtype == np.bool_ and stored.shape == scene["shape"] and np.array_equal(stored, ref["non_noise"])
    # an existing _mask.npy wins unless overridden
    fake = np.zeros(scene["shape"], bool)
    fake[1, 2, 3] = True
    np.save(mask_path, fake)
    assert np.array_equal(load_voxel_scene(path, "cuda:0")[1].cpu().numpy(), fake)
    other = load_voxel_scene(path, "cuda:0", recompute_mask=True, **{k: v for k, v in R.OTHER.items()})[1]
    assert np.array_equal(other.cpu().numpy(), ref_of("inexact24", "other")["non_noise"])
    with pytest.raises(ValueError):
        load_voxel_scene(path, "cuda:0", nb_neighbors=8)


def test_occupancy_points_metrics_on_scene64(tmp_path):
    """compute_occupancy_point_cloud's route: linspace axes over the bounds, eps = 5 * 0.01 on a lattice of spacing 1 / 63, the
    largest cluster"""
    from pixie_amd.occupancy import occupancy_points
    scene = dict(scene_of("scene64"))
    path = str(tmp_path / "clip_features.npz")
    lo, hi = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
    np.savez_compressed(path, min_bounds=lo, max_bounds=hi, voxel_size=1.0 / 64, feature_dim=4, grid_shape=scene["shape"])
    np.save(path.replace(".npz", "_alphas.npy"), scene["alphas"])
    np.save(path.replace(".npz", "_rgb.npy"), scene["rgb"])
    scene["axes"] = [torch.linspace(lo[a], hi[a], 64).numpy() for a in range(3)]
    scene["voxel_size"] = 0.01
    ref = R.reference(scene)
    xyz, rgb, metric = occupancy_points(path)
    assert metric["init_num_voxels"] == 64 ** 3 and tuple(metric["grid_shape"]) == (64, 64, 64)
    assert metric["num_voxels_after_density_threshold"] == ref["n_density"]
    assert metric["num_voxels_after_gray_background_filtering"] == metric["num_voxels_after_downsampling"] == ref["n_gray"]
    assert metric["num_voxels_after_outlier_removal"] == ref["n_stage_b"]
    assert metric["num_voxels_after_floating_cluster_removal"] == metric["final_num_voxels"] == int(ref["largest"].sum())
    want = R.coords_of(ref["largest"], scene["axes"]).astype(np.float32)
    assert np.array_equal(xyz.cpu().numpy(), want)
    assert np.array_equal(rgb.cpu().numpy(), scene["rgb"][ref["largest"]].astype(np.float32))
    with pytest.raises(ValueError):
        occupancy_points(path, voxel_downsample_size=0.02)


def test_argument_refusals():
    from pixie_amd import _lib
    from pixie_amd.occupancy import occupancy_mask, occupancy_points, load_voxel_scene
    scene = scene_of("few7")
    with pytest.raises(_lib.PixieHipError):
        occupancy_mask(scene["alphas"], scene["rgb"], scene["voxel_size"], device="cpu")
    with pytest.raises(_lib.PixieHipError):
        load_voxel_scene("nowhere.npz", "cpu")
    with pytest.raises(_lib.PixieHipError):
        occupancy_points("nowhere.npz", device="cpu")
    with pytest.raises(ValueError):
        run(scene, keep="biggest")
    with pytest.raises(ValueError):                                    # axes are host arrays: no read-back inside the call
        occupancy_mask(scene["alphas"], scene["rgb"], scene["voxel_size"], axes=[torch.from_numpy(a).cuda() for a in scene["axes"]])
    with pytest.raises(ValueError):
        occupancy_mask(scene["alphas"][:8], scene["rgb"], scene["voxel_size"])
    with pytest.raises(ValueError):
        occupancy_mask(scene["alphas"].astype(np.float64), scene["rgb"], scene["voxel_size"])
    for bad in (dict(nb_neighbors=0), dict(eps_multiplier=0.0), dict(eps_multiplier=-1.0), dict(min_cluster_pts=0), dict(eps_multiplier=40.0)):
        with pytest.raises(_lib.PixieHipError):
            run(scene, **bad)
    # the C ABI itself: null pointers and a dimension < 1 are refused with the library's error code before any launch
    lib = _lib.load()
    dev = torch.device("cuda:0")
    a = torch.zeros((4, 4, 4), dtype=torch.float16, device=dev)
    c = torch.zeros((4, 4, 4, 3), dtype=torch.float16, device=dev)
    ax = torch.arange(4, dtype=torch.float32, device=dev)
    out = torch.full((64,), 7, dtype=torch.uint8, device=dev)
    counts = torch.full((8,), -1, dtype=torch.int64, device=dev)
    scratch = torch.empty(1 << 20, dtype=torch.uint8, device=dev)

    def desc(**kw):
        d = _lib.OccupancyDesc()
        d.d_alphas, d.d_rgb, d.d_axis_x, d.d_axis_y, d.d_axis_z = a.data_ptr(), c.data_ptr(), ax.data_ptr(), ax.data_ptr(), ax.data_ptr()
        d.d, d.h, d.w, d.run_filters, d.nb_neighbors, d.min_points = 4, 4, 4, 1, 50, 10
        d.voxel_size = d.lattice_spacing = 1.0
        d.alpha_threshold, d.gray_threshold, d.std_ratio, d.eps_multiplier = 0.01, 0.05, 4.0, 5.0
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def call(d, mask=out, cnt=counts, scr=scratch):
        p = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)
        return lib.pixie_occupancy_mask(C.byref(d), p(mask), C.c_void_p(0), p(cnt), p(scr), C.c_void_p(0))

    assert 0 < lib.pixie_occupancy_scratch_bytes(C.byref(desc()), 1) < lib.pixie_occupancy_scratch_bytes(C.byref(desc()), 0) <= scratch.numel()
    assert lib.pixie_occupancy_scratch_bytes(C.byref(desc(h=0)), 0) == -1
    assert lib.pixie_occupancy_mask(None, C.c_void_p(out.data_ptr()), None, C.c_void_p(counts.data_ptr()), C.c_void_p(scratch.data_ptr()), None) != 0
    for d in (desc(d=0), desc(w=-3), desc(d_alphas=0), desc(d_rgb=0), desc(d_axis_y=0), desc(nb_neighbors=0), desc(eps_multiplier=0.0), desc(dtype=5),
              desc(keep=2)):
        assert call(d) != 0 and lib.pixie_last_error()
    assert call(desc(), mask=None) != 0 and call(desc(), cnt=None) != 0 and call(desc(), scr=None) != 0
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((counts == -1).all()), "a refused call launched nothing"
    assert call(desc()) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and counts.tolist() == [0] * 8


def test_mask_feeds_the_voxel_point_list():
    """end to end: the mask of scene64 goes into pixie_field_points, which lists exactly the voxels the stats object counts"""
    from pixie_amd.field_mapping import voxel_points
    scene = scene_of("scene64")
    mask, stats = run(scene, return_stats=True)
    pred = torch.zeros((11,) + scene["shape"], dtype=torch.float32, device="cuda")
    pts = voxel_points(pred, mask, (-0.5,) * 3, (0.5,) * 3)
    assert pts["xyz"].shape[0] == stats.counts["after_cluster_removal"] == int(ref_of("scene64", "defaults")["non_noise"].sum())
