"""GPU checks of the scene ingest (pixie_amd/scene_ingest.py -> pixie_scene_ingest, csrc/scene_ingest.hip) against the reference's
own run recorded in tests/golden/scene_ingest.npz and, at other sizes, against its NumPy restatement tests/_ingest_ref.py.
Bars: tests/_ingest_ref.py (exact classification, order and copies; floating quantities within 3 y of the float64 run)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pixie_amd import _lib
from tests import _ingest_ref as ir
from tests import _raster_ref as rr

pytestmark = pytest.mark.gpu

ROT2 = dict(rotation_degree=[30.0, -75.0], rotation_axis=[0, 2])
ROT0 = dict(rotation_degree=[], rotation_axis=[])
AREA = [-0.8, 0.75, -0.85, 0.7, -0.75, 0.8]
WIDE = [-5.0, 5.0, -5.0, 5.0, -5.0, 5.0]


def as_dict(scene):
    """an IngestedScene as host arrays under the golden's keys (the indices are not part of it: see kept_indices)"""
    h = lambda t: t.cpu().numpy()
    d = dict(pos=h(scene.pos), cov=h(scene.cov), opacity=h(scene.opacity), shs=h(scene.shs), scale_origin=np.float32(scene.scale_origin),
             original_mean_pos=h(scene.original_mean_pos))
    if scene.unselected is not None:
        d.update(unsel_pos=h(scene.unselected[0]), unsel_cov=h(scene.unselected[1]), unsel_opacity=h(scene.unselected[2]),
                 unsel_shs=h(scene.unselected[3]))
    return d


def kept_indices(got, ck, n_unsel_expected):
    """Which input rows the outputs are, recovered from the copies: every synthetic Gaussian has its own SH row, so the rows of
    `shs` identify the kept indices and their order."""
    from tests.test_scene_ingest_ply import fields
    shs = fields(ck)[4].reshape(len(ck), -1)
    key = {row.tobytes(): i for i, row in enumerate(shs)}
    assert len(key) == len(ck)
    got["sel_index"] = np.array([key.get(r.tobytes(), -1) for r in got["shs"].reshape(len(got["shs"]), -1)], np.int64)
    rows = got["unsel_shs"].reshape(len(got["unsel_shs"]), -1) if "unsel_shs" in got else np.zeros((0, shs.shape[1]), np.float32)
    got["unsel_index"] = np.array([key.get(r.tobytes(), -1) for r in rows], np.int64)
    return got


def run(ck, cfg, dev):
    from pixie_amd.scene_ingest import ingest_scene
    scene = ingest_scene(ck, cfg, device=dev)
    got = kept_indices(as_dict(scene), ck, None)
    assert scene.gs_num == len(got["sel_index"]) == scene.pos.shape[0]
    assert scene.n_loaded == len(ck) and scene.n_dropped == len(ck) - scene.gs_num - len(got["unsel_index"])
    return scene, got


@pytest.mark.parametrize("case", ir.CASES)
def test_golden_cases(hip_device, case):
    from pixie_amd.scene_ingest import load_gaussian_ply
    cfg = ir.golden_config(case)
    ck = load_gaussian_ply(ir.golden_ply(case), cfg["sh_degree"])
    _, f64, y = ir.golden_runs(case)
    scene, got = run(ck, cfg, hip_device)
    assert scene.gs_num == len(f64["sel_index"])
    ir.check_against(got, f64, y, f"device {case}")
    assert scene.z_shift_value == cfg["z_shift_value"] and len(scene.rotation_matrices) == len(cfg["rotation_degree"])


@pytest.mark.parametrize("n", [2, 255, 256, 257, 1000, 70000])
def test_sizes_rotations_area_shift_and_degree(hip_device, n):
    """0 and 2 rotations x with and without sim_area x z_shift 0 and 0.3 x SH degree 0 and 3, against the restatement: y is its
    float32-vs-float64 error on the same input.  70 000 rows span several scan tiles and 1094 emit workgroups; 255 / 256 / 257
    straddle the classify workgroup; 2 is the smallest selection with an extent."""
    from pixie_amd.scene_ingest import GaussianCheckpoint, generate_rotation_matrices
    for degree in (0, 3):
        k = (degree + 1) ** 2
        for rot in (ROT0, ROT2):
            for area in (None, WIDE if n == 2 else AREA):
                base = dict(rot, opacity_threshold=0.3, sim_area=area)
                block, names = ir.synthetic_block(n, k, 1000 + n + degree, base, all_selected=(n == 2))
                ck = GaussianCheckpoint(block, names, degree)
                mats = [m.numpy() for m in generate_rotation_matrices(rot["rotation_degree"], rot["rotation_axis"])]
                for z in (0.0, 0.3):
                    cfg = dict(base, z_shift_value=z)
                    r64 = ir.reference(block, ck.columns, k, cfg, np.float64)
                    r32 = ir.reference(block, ck.columns, k, cfg, np.float32, mats=mats)
                    assert r64["opacity_margin"] >= ir.MARGIN and r64["rotated_margin"] >= ir.MARGIN
                    y = {q: ir.rel(r32[q], r64[q]) for q in ir.FLOATING}
                    scene, got = run(ck, cfg, hip_device)
                    ir.check_against(got, r64, y, f"n {n} degree {degree} rotations {len(mats)} area {area is not None} z {z}")


def test_every_gaussian_selected(hip_device):
    from pixie_amd.scene_ingest import GaussianCheckpoint
    cfg = dict(ROT2, opacity_threshold=0.3, sim_area=WIDE, z_shift_value=0.0)
    block, names = ir.synthetic_block(500, 16, 3, cfg, all_selected=True)
    scene, got = run(GaussianCheckpoint(block, names, 3), cfg, hip_device)
    assert scene.gs_num == 500 and scene.n_dropped == 0 and scene.unselected is None
    assert scene.opacity_all.data_ptr() == scene.opacity.data_ptr() and scene.opacity_all.shape == scene.opacity.shape
    assert scene.shs_all.data_ptr() == scene.shs.data_ptr() and scene.shs_all.shape == scene.shs.shape
    assert np.array_equal(got["sel_index"], np.arange(500))


def test_opacity_filter_drops_all_but_two(hip_device):
    from pixie_amd.scene_ingest import GaussianCheckpoint
    cfg = dict(ROT2, opacity_threshold=0.3, sim_area=None, z_shift_value=0.3)
    block, names = ir.synthetic_block(3000, 16, 4, cfg, keep_only=2)
    ck = GaussianCheckpoint(block, names, 3)
    scene, got = run(ck, cfg, hip_device)
    r64 = ir.reference(block, ck.columns, 16, cfg, np.float64)
    assert scene.gs_num == 2 and scene.n_dropped == 2998 and np.array_equal(got["sel_index"], r64["sel_index"])
    ax = int(np.argmax(r64["pos"].max(axis=0) - r64["pos"].min(axis=0)))
    assert sorted(got["pos"][:, ax] - (0.3 if ax == 2 else 0.0)) == pytest.approx([0.5, 1.5], abs=1e-6)


def test_refusals_launch_nothing_afterwards(hip_device):
    from pixie_amd.scene_ingest import GaussianCheckpoint, ingest_scene
    cfg = dict(ROT2, opacity_threshold=0.3, sim_area=None, z_shift_value=0.0)
    block, names = ir.synthetic_block(400, 4, 5, cfg)
    ck = GaussianCheckpoint(block, names, 1)
    with pytest.raises(ValueError, match="nothing to simulate"):
        ingest_scene(ck, dict(cfg, sim_area=[5, 6, 5, 6, 5, 6]), device=hip_device)
    one, _ = ir.synthetic_block(400, 4, 5, cfg, keep_only=1)
    with pytest.raises(ValueError, match="zero extent"):
        ingest_scene(GaussianCheckpoint(one, names, 1), cfg, device=hip_device)
    with pytest.raises(ValueError, match="more than 8 rotations"):
        ingest_scene(ck, dict(cfg, rotation_degree=[10.0] * 9, rotation_axis=[0, 1, 2] * 3), device=hip_device)
    # the C entry point on the zero-extent input: the counts come back, the code is the documented one, no output row is written
    lib = _lib.load()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    n = 400
    blk = t(one)
    outs = [torch.full((n, w), float("nan"), device=hip_device) for w in (3, 6, 1, 12)]
    d = _lib.IngestDesc()
    d.n, d.n_attr, d.sh_degree, d.n_rotations, d.has_sim_area = n, one.shape[1], 1, 0, 0
    d.opacity_threshold, d.z_shift = 0.3, 0.0
    d.d_block, d.columns = blk.data_ptr(), ck.columns.ctypes.data_as(C.POINTER(C.c_int32))
    d.d_pos, d.d_cov, d.d_opacity, d.d_shs = (o.data_ptr() for o in outs)
    with torch.cuda.device(hip_device):
        ws = torch.empty(int(lib.pixie_scene_ingest_workspace_bytes(n)), dtype=torch.uint8, device=hip_device)
        d.d_workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        counts = (C.c_int64 * 3)()
        rc = lib.pixie_scene_ingest(C.byref(d), counts, None, None, _lib.current_stream_ptr())
        assert rc == _lib.INGEST_ZERO_EXTENT and list(counts) == [1, 0, 399] and b"zero extent" in lib.pixie_last_error()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(o).all()) for o in outs)
        d.n_rotations = 9
        assert lib.pixie_scene_ingest(C.byref(d), counts, None, None, _lib.current_stream_ptr()) == _lib.INGEST_TOO_MANY_ROTATIONS
        d.n_rotations, d.n = 0, 2 ** 31 - 1
        assert lib.pixie_scene_ingest(C.byref(d), counts, None, None, _lib.current_stream_ptr()) == _lib.INGEST_TOO_MANY_ROWS
        assert lib.pixie_scene_ingest_workspace_bytes(2 ** 31 - 1) == -1


def test_two_calls_give_the_same_bits_and_the_longest_axis_is_exact(hip_device):
    from pixie_amd.scene_ingest import GaussianCheckpoint, ingest_scene
    cfg = dict(ROT2, opacity_threshold=0.3, sim_area=AREA, z_shift_value=0.0)
    block, names = ir.synthetic_block(20000, 16, 6, cfg)
    ck = GaussianCheckpoint(block, names, 3)
    a, b = ingest_scene(ck, cfg, device=hip_device), ingest_scene(ck, cfg, device=hip_device)
    for x, y in zip((a.pos, a.cov, a.opacity_all, a.shs_all, a.unselected[0], a.unselected[1], a.original_mean_pos),
                    (b.pos, b.cov, b.opacity_all, b.shs_all, b.unselected[0], b.unselected[1], b.original_mean_pos)):
        assert torch.equal(x, y)
    assert a.scale_origin == b.scale_origin and a.gs_num == b.gs_num
    pos = a.pos.cpu().numpy()
    ax = int(np.argmax(pos.max(axis=0) - pos.min(axis=0)))
    assert pos[:, ax].min() == np.float32(0.5) and pos[:, ax].max() == np.float32(1.5)
    shifted = ingest_scene(ck, dict(cfg, z_shift_value=0.3), device=hip_device).pos.cpu().numpy()
    assert np.array_equal(shifted[:, :2], pos[:, :2]) and np.array_equal(shifted[:, 2], pos[:, 2] + np.float32(0.3))


@pytest.fixture(scope="module")
def thousand(hip_device):
    from pixie_amd.scene_ingest import GaussianCheckpoint, ingest_scene
    cfg = ir.golden_config("deg3")
    block, names = ir.synthetic_block(1000, 16, 7, cfg)
    ck = GaussianCheckpoint(block, names, 3)
    return ck, cfg, ingest_scene(ck, cfg, device=hip_device)


def test_plumbing_into_the_solver_and_back(hip_device, thousand):
    """IngestedScene -> load_initial_data_from_torch -> export_frame_for_rendering at step 0 returns the checkpoint's own selected
    positions and covariances, within 3 y of the reference's float32 round trip (golden case deg3, whose config this scene uses)"""
    from pixie_amd.mpm_solver import MPM_Simulator_WARP
    ck, cfg, scene = thousand
    g = ir.golden()
    sel = g["deg3/f64/sel_index"]
    y_pos = ir.rel(g["deg3/f32/roundtrip_pos"], g["deg3/f64/all_xyz"][sel])
    y_cov = ir.rel(g["deg3/f32/roundtrip_cov"], g["deg3/f64/all_cov"][sel])
    r64 = ir.reference(ck.block, ck.columns, 16, cfg, np.float64)
    assert scene.gs_num == len(r64["sel_index"]) > 200
    h = MPM_Simulator_WARP(10)
    h.load_initial_data_from_torch(scene.pos, torch.full((scene.gs_num,), 1e-6, device=hip_device), scene.cov, n_grid=32, grid_lim=2.5,
                                   device=str(hip_device))
    pos, cov = h.export_frame_for_rendering(scene.gs_num, scene.scale_origin, scene.original_mean_pos, scene.rotation_matrices,
                                            scene.z_shift_value)
    idx = torch.as_tensor(r64["sel_index"], device=hip_device)
    own_xyz, own_cov = ck.get_xyz[idx].cpu().numpy(), ck.get_covariance()[idx].cpu().numpy()
    e_pos, e_cov = ir.rel(pos.cpu().numpy(), own_xyz), ir.rel(cov.cpu().numpy(), own_cov)
    e_cov64 = ir.rel(cov.cpu().numpy(), r64["all_cov"][r64["sel_index"]])
    print(f"round trip: pos reference y {y_pos:.3e} ours {e_pos:.3e}; cov reference y {y_cov:.3e} ours {e_cov:.3e} "
          f"(against the float64 covariance {e_cov64:.3e})")
    assert e_pos <= ir.BAR * y_pos and e_cov <= ir.BAR * y_cov and e_cov64 <= ir.BAR * y_cov


def test_render_with_the_shared_buffers_equals_explicit_cats(hip_device, thousand):
    from pixie_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, convert_SH
    ck, cfg, scene = thousand
    r64 = ir.reference(ck.block, ck.columns, 16, cfg, np.float64)
    idx = torch.as_tensor(r64["sel_index"], device=hip_device)
    un = scene.unselected
    assert un is not None and scene.opacity_all.is_contiguous() and scene.shs_all.is_contiguous()
    assert scene.opacity_all.data_ptr() == scene.opacity.data_ptr() and scene.opacity_all.shape[0] == scene.gs_num + un[0].shape[0]
    means = torch.cat([ck.get_xyz[idx], un[0]], dim=0)
    cov = torch.cat([ck.get_covariance()[idx], un[1]], dim=0)
    cam = rr.look_at_camera((0.3, -0.4, -4.0), (0, 0, 0), 50.0, 96, 80)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    settings = GaussianRasterizationSettings(image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                             bg=t(np.array([0.1, 0.2, 0.3], np.float32)), scale_modifier=1.0, viewmatrix=t(cam["V"]),
                                             projmatrix=t(cam["P"]), sh_degree=3, campos=t(cam["campos"]), prefiltered=False, debug=False)
    view = SimpleNamespace(camera_center=t(cam["campos"]))
    r = GaussianRasterizer(settings)
    a, ra = r(means, None, scene.opacity_all, colors_precomp=convert_SH(scene.shs_all, view, ck, means), cov3D_precomp=cov)
    opacity_cat, shs_cat = torch.cat([scene.opacity, un[2]], dim=0), torch.cat([scene.shs, un[3]], dim=0)
    b, rb = r(means, None, opacity_cat, colors_precomp=convert_SH(shs_cat, view, ck, means), cov3D_precomp=cov)
    assert torch.equal(a, b) and torch.equal(ra, rb) and int((ra > 0).sum()) > 100
    assert float((a - t(np.array([0.1, 0.2, 0.3], np.float32))[:, None, None]).abs().max()) > 0.05     # something was drawn
