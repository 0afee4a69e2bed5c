"""GPU tests of the batched rasteriser (pixie_raster_forward_batch, FrameBatchRasterizer, render_frame_batch): every image, radius,
final_T and n_contrib of a batch is bit-equal (torch.equal) to the per-view GaussianRasterizer call, which tests/test_raster_hip.py
pins against the NumPy helper.  Scenes and cameras come from tests/_raster_ref.py; the per-view references of a scene are computed
once and shared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pixie_amd import _lib
from tests import _raster_ref as rr

pytestmark = pytest.mark.gpu


def tens(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


def make_settings(cam, bg, dev, sh_degree=0):
    from pixie_amd.rasterizer import GaussianRasterizationSettings
    return GaussianRasterizationSettings(image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                         bg=tens(bg, dev), scale_modifier=1.0, viewmatrix=tens(cam["V"], dev), projmatrix=tens(cam["P"], dev),
                                         sh_degree=sh_degree, campos=tens(cam["campos"], dev), prefiltered=False, debug=False)


def orbit(cam, degrees):
    """The scene's camera moved round the origin's y axis, looking at the origin as every scene camera does."""
    a = np.radians(degrees)
    e = cam["campos"].astype(np.float64)
    eye = (np.cos(a) * e[0] + np.sin(a) * e[2], e[1], -np.sin(a) * e[0] + np.cos(a) * e[2])
    return rr.look_at_camera(eye, (0, 0, 0), float(np.degrees(2 * np.arctan(cam["tanfovx"]))), cam["W"], cam["H"])


def looking_away(cam):
    """From three times as far, with the whole scene behind the camera (as scene f is set up): everything is culled at the near plane."""
    e = cam["campos"].astype(np.float64)
    return rr.look_at_camera(3 * e, 6 * e, float(np.degrees(2 * np.arctan(cam["tanfovx"]))), cam["W"], cam["H"])


@functools.lru_cache(maxsize=None)
def case(name, views, dev_str, away=None):
    """Scene `name` seen by `views` cameras (its own, then orbits of it; view `away` looks away), means jittered per view by a seeded
    1 %: device tensors, the settings, and the per-view GaussianRasterizer results with their instance counts."""
    from pixie_amd.rasterizer import GaussianRasterizer
    dev = torch.device(dev_str)
    s = rr.scene(name)
    cam0 = s["cam"]
    cams = [cam0] + [orbit(cam0, 25.0 * k * (-1) ** k) for k in range(1, views)]
    if away is not None:
        cams[away] = looking_away(cam0)
    rng = np.random.default_rng(1000 + len(name) + views)
    n = len(s["means"])
    means = np.stack([s["means"] * (1.0 + 0.01 * rng.uniform(-1, 1, (n, 3))) for _ in range(views)]).astype(np.float32)
    cov = rr.cov3d_from_scale_rot(s["scales"], s["rotations"], 1.0, np.float32).reshape(n, 6)
    c = dict(s=s, cams=cams, n=n, means=tens(means, dev), cov=tens(np.stack([cov] * views), dev), opacity=tens(s["opacity"], dev),
             colors=tens(s["colors"].reshape(n, 3), dev), settings=[make_settings(cm, s["bg"], dev) for cm in cams], bg=s["bg"])
    c["ref"], c["instances"] = [], []
    for v in range(views):
        single = GaussianRasterizer(c["settings"][v])
        c["ref"].append(single(c["means"][v], None, c["opacity"], colors_precomp=c["colors"], cov3D_precomp=c["cov"][v], aux=True))
        c["instances"].append(single.last_instances)
    return c


def assert_view_equal(got, v, ref, tag):
    color, radii, final_T, n_contrib = ref
    assert torch.equal(got.color[v], color), f"{tag}: color of view {v}"
    assert torch.equal(got.radii[v], radii), f"{tag}: radii of view {v}"
    assert torch.equal(got.final_T[v], final_T), f"{tag}: final_T of view {v}"
    assert torch.equal(got.n_contrib[v], n_contrib), f"{tag}: n_contrib of view {v}"


def batch_of(c, **kw):
    from pixie_amd.rasterizer import FrameBatchRasterizer
    r = FrameBatchRasterizer()
    return r, r(c["means"], c["cov"], c["settings"], c["opacity"], colors_precomp=c["colors"], aux=True, **kw)


@pytest.mark.parametrize("name", ["a", "d", "g", "i"])
def test_every_view_is_bit_equal_to_the_single_call(hip_device, name):
    c = case(name, 3, str(hip_device))
    r, got = batch_of(c)
    assert got.color.shape == (3, 3, c["cams"][0]["H"], c["cams"][0]["W"]) and got.radii.shape == (3, c["n"])
    for v in range(3):
        assert_view_equal(got, v, c["ref"][v], name)
    assert not torch.equal(got.color[0], got.color[1]) and not torch.equal(got.color[1], got.color[2])
    assert r.last_instances == c["instances"] and all(k > 0 for k in r.last_instances) and 1 <= r.last_groups <= 3


def test_an_empty_view_between_two_full_ones(hip_device):
    c = case("a", 3, str(hip_device), away=1)
    r, got = batch_of(c)
    for v in range(3):
        assert_view_equal(got, v, c["ref"][v], "a, middle view away")
    bg = tens(c["bg"], hip_device)
    assert r.last_instances[1] == 0 and r.last_instances[0] > 0 and r.last_instances[2] > 0
    assert torch.equal(got.color[1], bg[:, None, None].expand_as(got.color[1])) and int(got.radii[1].abs().sum()) == 0
    assert torch.equal(got.final_T[1], torch.ones_like(got.final_T[1])) and int(got.n_contrib[1].abs().sum()) == 0


def test_no_gaussian_and_one_view(hip_device):
    c = case("h", 2, str(hip_device))
    r, got = batch_of(c)
    bg = tens(c["bg"], hip_device)
    assert c["n"] == 0 and r.last_instances == [0, 0] and r.last_groups == 1 and got.radii.shape == (2, 0)
    for v in range(2):
        assert torch.equal(got.color[v], bg[:, None, None].expand_as(got.color[v]))
        assert_view_equal(got, v, c["ref"][v], "h")
    c = case("i", 1, str(hip_device))
    r, got = batch_of(c)
    assert_view_equal(got, 0, c["ref"][0], "i, one view")
    assert r.last_groups == 1 and len(r.last_instances) == 1


@pytest.mark.parametrize("name", ["b", "e"])
def test_partial_tiles_and_one_gaussian_over_every_tile(hip_device, name):
    c = case(name, 2, str(hip_device))
    W, H = c["cams"][0]["W"], c["cams"][0]["H"]
    assert (W, H) == ((250, 187) if name == "b" else (112, 80))
    r, got = batch_of(c)
    for v in range(2):
        assert_view_equal(got, v, c["ref"][v], name)
    if name == "e":
        assert r.last_instances[0] == ((W + 15) // 16) * ((H + 15) // 16)      # the one Gaussian is in every tile


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_colours_in_the_projection_kernel(hip_device, degree):
    from pixie_amd.rasterizer import FrameBatchRasterizer, GaussianRasterizer, sh_to_rgb
    c = case("d", 3, str(hip_device))
    shs = tens(np.random.default_rng(77).normal(0.0, 0.4, (c["n"], 16, 3)).astype(np.float32), hip_device)
    settings = [make_settings(cm, c["bg"], hip_device, sh_degree=degree) for cm in c["cams"]]
    assert len({tuple(cm["campos"].tolist()) for cm in c["cams"]}) == 3
    got = FrameBatchRasterizer()(c["means"], c["cov"], settings, c["opacity"], shs=shs, aux=True)
    images = []
    for v in range(3):
        colors = sh_to_rgb(shs, degree, c["means"][v], settings[v].campos)
        ref = GaussianRasterizer(settings[v])(c["means"][v], None, c["opacity"], colors_precomp=colors, cov3D_precomp=c["cov"][v], aux=True)
        assert_view_equal(got, v, ref, f"SH degree {degree}")
        images.append(ref[0])
    assert not torch.equal(images[0], c["ref"][0][0])
    if degree > 0:                                    # the colour depends on where the camera stands
        one = sh_to_rgb(shs, degree, c["means"][1], settings[0].campos)
        assert not torch.equal(one, sh_to_rgb(shs, degree, c["means"][1], settings[1].campos))


def test_static_tail(hip_device):
    from pixie_amd.rasterizer import FrameBatchRasterizer, GaussianRasterizer
    c = case("d", 3, str(hip_device))
    m, rng = 300, np.random.default_rng(9)
    extra = (tens(rng.normal(size=(m, 3)).astype(np.float32) * 0.4, hip_device),
             tens(np.tile(np.array([[2e-3, 1e-4, 0, 1e-3, 0, 3e-3]], np.float32), (m, 1)), hip_device))
    op2 = torch.cat([c["opacity"], tens(rng.uniform(0.3, 0.9, m).astype(np.float32), hip_device)])
    col2 = torch.cat([c["colors"], tens(rng.uniform(0, 1, (m, 3)).astype(np.float32), hip_device)])
    r = FrameBatchRasterizer()
    got = r(c["means"], c["cov"], c["settings"], op2, colors_precomp=col2, static=extra, aux=True)
    assert got.radii.shape == (3, c["n"] + m)
    for v in range(3):
        ref = GaussianRasterizer(c["settings"][v])(torch.cat([c["means"][v], extra[0]]), None, op2, colors_precomp=col2,
                                                   cov3D_precomp=torch.cat([c["cov"][v], extra[1]]), aux=True)
        assert_view_equal(got, v, ref, "static tail")
        assert not torch.equal(got.color[v], c["ref"][v][0]) and int((got.radii[v, c["n"]:] > 0).sum()) > 0
    # per-view colours (a view stride) give what shared ones give
    per_view = r(c["means"], c["cov"], c["settings"], op2, colors_precomp=col2[None].repeat(3, 1, 1), static=extra, aux=True)
    assert torch.equal(per_view.color, got.color)
    # the static tail alone (no dynamic Gaussian)
    alone = r(c["means"][:, :0], c["cov"][:, :0], c["settings"], op2[c["n"]:], colors_precomp=col2[c["n"]:], static=extra, aux=True)
    ref = GaussianRasterizer(c["settings"][2])(extra[0], None, op2[c["n"]:], colors_precomp=col2[c["n"]:], cov3D_precomp=extra[1], aux=True)
    assert_view_equal(alone, 2, ref, "static tail alone")


def raw_batch(c, dev, capacity, fill=7.0):
    """One pixie_raster_forward_batch through the C ABI with a workspace sized for `capacity` instances and outputs pre-filled."""
    lib = _lib.load()
    V, n, W, H = len(c["cams"]), c["n"], c["cams"][0]["W"], c["cams"][0]["H"]
    views = (_lib.RasterView * V)()
    for v, cam in enumerate(c["cams"]):
        views[v].viewmatrix = (C.c_float * 16)(*cam["V"].reshape(-1).tolist())
        views[v].projmatrix = (C.c_float * 16)(*cam["P"].reshape(-1).tolist())
        views[v].campos = (C.c_float * 3)(*cam["campos"].tolist())
        views[v].tanfovx, views[v].tanfovy = cam["tanfovx"], cam["tanfovy"]
    out = torch.full((V, 3, H, W), fill, device=dev)
    rgb8 = torch.full((V, H, W, 3), 7, dtype=torch.uint8, device=dev)
    fT = torch.full((V, H, W), fill, device=dev)
    nc = torch.full((V, H, W), 7, dtype=torch.int32, device=dev)
    radii = torch.full((V, n), -7, dtype=torch.int32, device=dev)
    d = _lib.RasterBatchDesc()
    d.views, d.n_dyn, d.n_static, d.width, d.height, d.scale_modifier = V, n, 0, W, H, 1.0
    d.bg = (C.c_float * 3)(*c["bg"].tolist())
    d.view = views
    d.d_means, d.d_cov3d, d.means_view_stride, d.cov3d_view_stride = c["means"].data_ptr(), c["cov"].data_ptr(), n * 3, n * 6
    d.d_opacity, d.d_colors = c["opacity"].data_ptr(), c["colors"].data_ptr()
    d.d_out_color, d.d_out_rgb8, d.d_radii, d.d_final_T, d.d_n_contrib = out.data_ptr(), rgb8.data_ptr(), radii.data_ptr(), fT.data_ptr(), nc.data_ptr()
    nb = lib.pixie_raster_batch_workspace_bytes(n, V, W, H, capacity)
    assert nb >= 0, lib.pixie_last_error()
    ws = torch.full((nb + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    d.d_workspace, d.workspace_bytes, d.max_instances = ws.data_ptr(), nb, capacity
    counts, groups = (C.c_int64 * V)(), C.c_int32(-1)
    rc = lib.pixie_raster_forward_batch(C.byref(d), counts, C.byref(groups), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    assert (ws[nb:] == 0xA5).all(), "the workspace's canary tail was written"
    return dict(rc=rc, error=lib.pixie_last_error().decode(), counts=list(counts), groups=groups.value, color=out, rgb8=rgb8, radii=radii,
                final_T=fT, n_contrib=nc)


def test_groups(hip_device):
    from pixie_amd.rasterizer import FrameBatchRasterizer
    c = case("a", 3, str(hip_device))
    counts = c["instances"]
    r, one = batch_of(c, capacity=sum(counts))
    assert r.last_groups == 1 and r.last_instances == counts      # a workspace sized for all views: one sort
    largest = max(counts)
    assert sum(counts) > largest + 1
    r2 = FrameBatchRasterizer()
    many = r2(c["means"], c["cov"], c["settings"], c["opacity"], colors_precomp=c["colors"], aux=True, capacity=largest + 1)
    assert r2.last_groups > 1 and r2.last_instances == counts
    for a, b in zip(many, one):
        assert b is None or torch.equal(a, b)
    for v in range(3):
        assert_view_equal(many, v, c["ref"][v], "one view per group")

    # the C call with room for all, for two groups, and for less than the largest view
    full = raw_batch(c, hip_device, sum(counts))
    assert full["rc"] == 0 and full["groups"] == 1 and full["counts"] == counts, full["error"]
    assert torch.equal(full["color"], one.color) and torch.equal(full["radii"], one.radii)
    assert torch.equal(full["final_T"], one.final_T) and torch.equal(full["n_contrib"], one.n_contrib)
    tight = raw_batch(c, hip_device, largest)
    assert tight["rc"] == 0 and tight["groups"] > 1 and torch.equal(tight["color"], one.color) and torch.equal(tight["rgb8"], full["rgb8"])
    short = raw_batch(c, hip_device, largest - 1)
    v = counts.index(largest)
    assert short["rc"] != 0 and str(largest) in short["error"] and f"view {v} " in short["error"], short["error"]
    assert short["counts"] == counts and torch.equal(short["radii"], one.radii) and short["groups"] == 0
    assert bool((short["color"] == 7.0).all()) and bool((short["final_T"] == 7.0).all())
    assert bool((short["rgb8"] == 7).all()) and bool((short["n_contrib"] == 7).all())

    # the Python wrapper grows once and succeeds
    r3 = FrameBatchRasterizer()
    grown = r3(c["means"], c["cov"], c["settings"], c["opacity"], colors_precomp=c["colors"], aux=True, capacity=largest - 1)
    assert r3.last_instances == counts and r3._capacity >= largest and r3.last_groups >= 1
    assert torch.equal(grown.color, one.color) and torch.equal(grown.n_contrib, one.n_contrib)


@pytest.mark.parametrize("name,bg", [("a", None), ("d", (1.0, 0.7, 0.0031))])
def test_uint8_frames(hip_device, tmp_path, name, bg):
    from pixie_amd.rasterizer import FrameBatchRasterizer, render_frame_batch, save_frame_pngs
    c = case(name, 3, str(hip_device))
    bg = c["bg"] if bg is None else np.array(bg, np.float32)
    settings = [make_settings(cm, bg, hip_device) for cm in c["cams"]]
    got = FrameBatchRasterizer()(c["means"], c["cov"], settings, c["opacity"], colors_precomp=c["colors"], out_rgb8=True, out=True)
    assert got.rgb8.dtype == torch.uint8 and got.rgb8.shape == (3, c["cams"][0]["H"], c["cams"][0]["W"], 3)
    want = (got.color * 255.0).clamp(0.0, 255.0).round().to(torch.uint8).permute(0, 2, 3, 1)
    assert torch.equal(got.rgb8, want)
    assert len(torch.unique(want)) > 50               # a real image, not a flat one
    frames = (c["means"], c["cov"])
    only = render_frame_batch(frames, settings, c["opacity"], colors_precomp=c["colors"], out_rgb8=True)
    assert only.dtype == torch.uint8 and torch.equal(only, want)
    assert torch.equal(render_frame_batch(frames, settings, c["opacity"], colors_precomp=c["colors"], frames_per_call=2), got.color)
    try:
        from PIL import Image
    except ImportError:
        with pytest.raises(RuntimeError, match="needs Pillow"):
            save_frame_pngs(str(tmp_path), only)
        return
    paths = save_frame_pngs(str(tmp_path / "frames"), only, start=4)
    assert [p[-9:] for p in paths] == ["00004.png", "00005.png", "00006.png"]
    for f, p in enumerate(paths):
        assert np.array_equal(np.asarray(Image.open(p).convert("RGB")), want[f].cpu().numpy())
    again = save_frame_pngs(str(tmp_path / "floats"), got.color)
    assert np.array_equal(np.asarray(Image.open(again[2]).convert("RGB")), want[2].cpu().numpy())


def test_hand_off_from_run_frames(hip_device):
    from pixie_amd import rasterizer as R
    from pixie_amd.mpm_solver import FrameSchedule, SceneBatch
    from pixie_amd.synthetic import mpm_ball_scene
    from tests.test_mpm_batch_hip import make
    n = 5000
    solver = make(mpm_ball_scene(n, seed=1, n_grid=32, scenario="tree"))
    with SceneBatch([solver]) as sb:
        frames = sb.run_frames([FrameSchedule(1e-4, 60, 3, gs_num=n)])[0]
    pos, cov = frames[0], frames[1]
    cam = rr.look_at_camera((0.0, -2.4, 0.3), (0.0, 0.0, 0.0), 40.0, 168, 120, up=(0.0, 0.0, -1.0))
    rng = np.random.default_rng(2)
    opacity = tens(rng.uniform(0.2, 1.0, n).astype(np.float32), hip_device)
    colors = tens(rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32), hip_device)
    settings = make_settings(cam, np.ones(3, np.float32), hip_device)
    images = R.render_frames(frames, settings, opacity, colors_precomp=colors)
    assert torch.equal(R.render_frames(frames, settings, opacity, colors_precomp=colors, batch=True), images)
    r = R.FrameBatchRasterizer()
    assert torch.equal(R.render_frames(frames, [settings] * 3, opacity, colors_precomp=colors, batch=r), images)
    assert len(r.last_instances) == 3 and r.last_groups >= 1 and not torch.equal(images[1], images[0])
    # slices of the sequence go to the library as they lie in memory
    for sl in (slice(1, 3), slice(0, 3, 2)):
        p, c6 = pos[sl], cov[sl]
        kept, stride = R._view_f32(p, "pos", n, 3)
        assert kept.data_ptr() == p.data_ptr() and stride == p.stride(0) and R._view_f32(c6, "cov", n, 6)[0].data_ptr() == c6.data_ptr()
        assert torch.equal(r(p, c6, settings, opacity, colors_precomp=colors).color, images[sl])
    # unselected Gaussians ride along without a concatenation per frame
    m = 300
    extra = (tens(rng.normal(size=(m, 3)).astype(np.float32) * 0.2, hip_device),
             tens(np.tile(np.array([[4e-4, 0, 0, 4e-4, 0, 4e-4]], np.float32), (m, 1)), hip_device))
    op2, col2 = torch.cat([opacity, torch.full((m,), 0.7, device=hip_device)]), torch.cat([colors, torch.zeros((m, 3), device=hip_device)])
    with_extra = R.render_frames(frames, settings, op2, colors_precomp=col2, unselected=extra)
    assert torch.equal(R.render_frame_batch(frames, settings, op2, colors_precomp=col2, unselected=extra), with_extra)
    assert not torch.equal(with_extra, images)
