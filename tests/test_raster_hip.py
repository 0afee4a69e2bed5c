"""GPU tests of the forward 3DGS rasteriser (pixie_raster_forward, pixie_sh_to_rgb, pixie_amd/rasterizer.py) against the NumPy
helper tests/_raster_ref.py on its scenes (a) ... (i).

Bars, per scene.  `radii`: equal to the float64 helper off the borderline Gaussians.  Pixels: let y be the largest absolute pixel
difference between the helper's float32 and float64 runs off the borderline pixels (computed here); the HIP image must lie within
3 y of the float64 run on the same pixels -- device exp, rcp and sqrt are good to 1-2 ulp where NumPy's are correctly rounded to
about half an ulp.  final_T on the same terms, n_contrib exactly, off the borderline pixels.  Borderline pixels: finite and within
[0, max(colours, bg)].  Every raw launch writes into NaN-filled outputs and a workspace with a canary tail, and is launched twice:
the two results are bit-equal.  The observed error / y per scene is printed (and appended to $PIXIE_RASTER_PARITY_OUT if set)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pixie_amd import _lib
from tests import _raster_ref as rr

pytestmark = pytest.mark.gpu
CANARY = 4096


def raw_forward(s, dev, cov6=None, colors=None, instances=None, expect_fail=False):
    """One pixie_raster_forward through the C ABI.  instances: size the workspace for that many (default: ask with a probe call that
    is allowed to fail).  Returns dict(color, radii, final_T, n_contrib, count, rc)."""
    lib = _lib.load()
    cam = s["cam"]
    W, H, n = cam["W"], cam["H"], len(s["means"])
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)
    means, opac = t(s["means"]), t(s["opacity"])
    cols = t(s["colors"] if colors is None else colors)
    cov = t(cov6) if cov6 is not None else None
    sc, rot = (None, None) if cov6 is not None else (t(s["scales"]), t(s["rotations"]))
    out = torch.full((3, H, W), float("nan"), device=dev)
    fT = torch.full((H, W), float("nan"), device=dev)
    nc = torch.full((H, W), -7, dtype=torch.int32, device=dev)
    radii = torch.full((n,), -7, dtype=torch.int32, device=dev)
    d = _lib.RasterDesc()
    d.n, d.width, d.height = n, W, H
    d.tanfovx, d.tanfovy, d.scale_modifier = cam["tanfovx"], cam["tanfovy"], s["scale_modifier"]
    d.viewmatrix = (C.c_float * 16)(*cam["V"].reshape(-1).tolist())
    d.projmatrix = (C.c_float * 16)(*cam["P"].reshape(-1).tolist())
    d.bg = (C.c_float * 3)(*s["bg"].tolist())
    for name, x in (("d_means", means), ("d_cov3d", cov), ("d_scales", sc), ("d_rotations", rot), ("d_colors", cols), ("d_opacity", opac),
                    ("d_radii", radii)):
        setattr(d, name, x.data_ptr() if x is not None and x.numel() else None)
    d.d_out_color, d.d_final_T, d.d_n_contrib = out.data_ptr(), fT.data_ptr(), nc.data_ptr()
    count = C.c_int64(-1)
    st = _lib.current_stream_ptr()
    if instances is None:                      # probe: a workspace for zero instances reports the count (or succeeds when it is 0)
        nb = lib.pixie_raster_workspace_bytes(n, W, H, 0)
        assert nb >= 0, lib.pixie_last_error()
        ws = torch.empty((nb + CANARY,), dtype=torch.uint8, device=dev)
        d.d_workspace, d.workspace_bytes = ws.data_ptr(), nb
        lib.pixie_raster_forward(C.byref(d), C.byref(count), st)
        instances = count.value
        out.fill_(float("nan")); fT.fill_(float("nan")); nc.fill_(-7); radii.fill_(-7)
    nb = lib.pixie_raster_workspace_bytes(n, W, H, instances)
    assert nb >= 0, lib.pixie_last_error()
    ws = torch.full((nb + CANARY,), 0xA5, dtype=torch.uint8, device=dev)
    d.d_workspace, d.workspace_bytes = ws.data_ptr(), nb
    rc = lib.pixie_raster_forward(C.byref(d), C.byref(count), st)
    torch.cuda.synchronize()
    assert (ws[nb:] == 0xA5).all(), "the workspace's canary tail was written"
    if not expect_fail:
        assert rc == 0, lib.pixie_last_error()
    return dict(color=out.cpu().numpy(), radii=radii.cpu().numpy(), final_T=fT.cpu().numpy(), n_contrib=nc.cpu().numpy(), count=count.value,
                rc=rc, error=lib.pixie_last_error().decode())


def record(line):
    print(line)
    path = os.environ.get("PIXIE_RASTER_PARITY_OUT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def tile_sample(s, share, seed):
    cam = s["cam"]
    ty, tx = (cam["H"] + 15) // 16, (cam["W"] + 15) // 16
    return np.random.default_rng(seed).random((ty, tx)) < share


def check_against_helper(s, got, tag, cov6=None, tile_mask=None):
    r64, r32, y = rr.yardstick(s, cov6=cov6, tile_mask=tile_mask)
    bp, bgau, sel = r64["borderline_pixels"], r64["borderline_gaussians"], r64["selected"]
    assert bp.sum() <= 0.005 * sel.sum() and bgau.sum() <= 0.005 * max(len(bgau), 1), f"{tag}: the scene is not fit to compare on"
    assert np.array_equal(got["radii"][~bgau], r64["radii"][~bgau]), f"{tag}: radii"
    assert y <= rr.Y_CAP, f"{tag}: yardstick y = {y:.3e}: a float32 / float64 decision flip escaped the borderline sets"
    keep = sel & ~bp
    assert np.isfinite(got["color"]).all() and np.isfinite(got["final_T"]).all(), f"{tag}: an output pixel was not written"
    err = float(np.max(np.abs(got["color"].astype(np.float64) - r64["color"])[:, keep], initial=0.0))
    yT = float(np.max(np.abs(r32["final_T"].astype(np.float64) - r64["final_T"])[keep], initial=0.0))
    errT = float(np.max(np.abs(got["final_T"].astype(np.float64) - r64["final_T"])[keep], initial=0.0))
    ratio = lambda e, yy: (e / yy) if yy > 0 else (0.0 if e == 0 else float("inf"))
    record(f"scene {tag}: {len(bgau)} Gaussians, {s['cam']['W']}x{s['cam']['H']}, {got['count']} instances, pixels compared {int(keep.sum())}, "
           f"borderline pixels {int(bp.sum())}, y {y:.3e}, HIP error {err:.3e} = {ratio(err, y):.2f} y; final_T y {yT:.3e}, "
           f"HIP error {errT:.3e} = {ratio(errT, yT):.2f} y")
    assert err <= 3 * y, f"{tag}: pixel error {err:.3e} exceeds 3 y = {3 * y:.3e}"
    assert errT <= 3 * yT, f"{tag}: final_T error {errT:.3e} exceeds 3 y = {3 * yT:.3e}"
    assert np.array_equal(got["n_contrib"][keep], r64["n_contrib"][keep]), f"{tag}: n_contrib"
    top = max(float(np.max(s["colors"], initial=0.0)), float(s["bg"].max()))
    b = got["color"][:, bp & sel]
    assert np.isfinite(b).all() and (b >= 0).all() and (b <= top).all(), f"{tag}: borderline pixels outside [0, {top}]"
    return r64


@pytest.mark.parametrize("name", rr.SCENES)
def test_scene_against_the_helper(hip_device, name):
    s = rr.scene(name)
    got = raw_forward(s, hip_device)
    again = raw_forward(s, hip_device, instances=got["count"])
    for k in ("color", "radii", "final_T", "n_contrib"):
        assert np.array_equal(got[k], again[k]), f"{name}: two launches differ in {k}"
    mask = tile_sample(s, 0.05, 5) if name == "c" else None
    r64 = check_against_helper(s, got, name, tile_mask=mask)
    cam = s["cam"]
    if name in ("f", "h"):
        assert got["count"] == 0 and (got["radii"] == 0).all()
        assert np.array_equal(got["color"], np.broadcast_to(s["bg"][:, None, None], got["color"].shape))
        assert (got["final_T"] == 1).all() and (got["n_contrib"] == 0).all()
    if name == "b":
        assert cam["W"] % 16 and cam["H"] % 16
    if name == "e":
        assert got["count"] == ((cam["W"] + 15) // 16) * ((cam["H"] + 15) // 16)
    if name == "i":
        assert got["n_contrib"].max() > 2 * 256
    if name == "d":
        assert (got["final_T"] < 0.011).mean() > 0.2
    if name == "g":
        assert 0 < (got["radii"] > 0).sum() < len(got["radii"])


def test_cov3d_route_and_scale_rotation_route(hip_device):
    """the scales / rotations route equals, bit for bit, the cov3D_precomp route fed with the covariances the helper builds in float32:
    raster_math.h builds the covariance in the helper's order of operations and raster.hip is compiled without contraction, so the
    two routes hand project() the same six floats; the cov3D route also meets the bars against the helper"""
    s = rr.scene("a")
    c32 = rr.cov3d_from_scale_rot(s["scales"], s["rotations"], s["scale_modifier"], np.float32)
    by_cov = raw_forward(s, hip_device, cov6=c32)
    check_against_helper(s, by_cov, "a/cov3d", cov6=c32)
    by_sr = raw_forward(s, hip_device)
    assert by_cov["count"] == by_sr["count"]
    for k in ("color", "radii", "final_T", "n_contrib"):
        assert np.array_equal(by_cov[k], by_sr[k]), f"the two routes differ in {k}"


def test_small_workspace_is_refused_and_the_wrapper_grows(hip_device):
    from pixie_amd.rasterizer import GaussianRasterizer
    s = rr.scene("a")
    full = raw_forward(s, hip_device)
    count = full["count"]
    assert count > 1000
    small = raw_forward(s, hip_device, instances=count // 2, expect_fail=True)
    assert small["rc"] != 0 and small["count"] == count and str(count) in small["error"] and "too small" in small["error"]
    assert np.isnan(small["color"]).all() and np.isnan(small["final_T"]).all() and (small["n_contrib"] == -7).all()    # nothing rendered
    assert np.array_equal(small["radii"], full["radii"])          # step 1 ran: radii are its output
    r = GaussianRasterizer(settings_of(s, hip_device))
    lib = _lib.load()
    t = lambda a: torch.from_numpy(a).to(hip_device)
    with torch.cuda.device(hip_device):
        r._ensure_workspace(lib, len(s["means"]), hip_device, 8)
    assert r._capacity == 8
    color, radii = r(t(s["means"]), None, t(s["opacity"])[:, None], colors_precomp=t(s["colors"]), scales=t(s["scales"]), rotations=t(s["rotations"]))
    assert r._capacity == count + count // 2 and r.last_instances == count
    assert np.array_equal(color.cpu().numpy(), full["color"]) and np.array_equal(radii.cpu().numpy(), full["radii"])
    ws = r._workspace
    color2, _, fT, nc = r(t(s["means"]), None, t(s["opacity"]), colors_precomp=t(s["colors"]), scales=t(s["scales"]), rotations=t(s["rotations"]),
                          aux=True)
    assert r._workspace is ws and torch.equal(color, color2)      # kept between calls
    assert np.array_equal(fT.cpu().numpy(), full["final_T"]) and np.array_equal(nc.cpu().numpy(), full["n_contrib"])


def settings_of(s, dev, sh_degree=0):
    from pixie_amd.rasterizer import GaussianRasterizationSettings
    cam = s["cam"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return GaussianRasterizationSettings(image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                         bg=t(s["bg"]), scale_modifier=s["scale_modifier"], viewmatrix=t(cam["V"]), projmatrix=t(cam["P"]),
                                         sh_degree=sh_degree, campos=t(cam["campos"]), prefiltered=False, debug=False)


def test_shs_route_equals_convert_sh_plus_colors(hip_device):
    from types import SimpleNamespace
    from pixie_amd.rasterizer import GaussianRasterizer, convert_SH, sh_to_rgb
    s = rr.scene("a")
    n = len(s["means"])
    rng = np.random.default_rng(3)
    shs_np = (rng.normal(size=(n, 16, 3)) * 0.4).astype(np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    shs, means, opac, sc, rot = t(shs_np), t(s["means"]), t(s["opacity"]), t(s["scales"]), t(s["rotations"])
    cam = SimpleNamespace(camera_center=t(s["cam"]["campos"]))
    dirs = s["means"].astype(np.float64) - s["cam"]["campos"].astype(np.float64)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    for degree in range(4):
        pc = SimpleNamespace(max_sh_degree=3, active_sh_degree=degree)
        cols = convert_SH(shs, cam, pc, means)
        assert cols.shape == (n, 3) and cols.dtype == torch.float32
        assert np.allclose(cols.cpu().numpy(), rr.eval_sh64(shs_np, degree, dirs), rtol=0, atol=1e-5), degree
        r = GaussianRasterizer(settings_of(s, hip_device, sh_degree=degree))
        a, ra = r(means, None, opac, shs=shs, scales=sc, rotations=rot)
        b, rb = r(means, None, opac, colors_precomp=cols, scales=sc, rotations=rot)
        assert torch.equal(a, b) and torch.equal(ra, rb), degree
    # a per-Gaussian rotation of the first n_rot directions
    n_rot = 1234
    q = rng.normal(size=(n_rot, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1).reshape(n_rot, 3, 3)
    d2 = dirs.copy()
    d2[:n_rot] = np.einsum("nij,nj->ni", R, dirs[:n_rot])
    cols = sh_to_rgb(shs, 3, means, cam.camera_center, rotation=t(R.astype(np.float32)))
    assert np.allclose(cols.cpu().numpy(), rr.eval_sh64(shs_np, 3, d2), rtol=0, atol=1e-5)
    with pytest.raises(ValueError, match="no CPU path"):
        convert_SH(shs.cpu(), cam, SimpleNamespace(max_sh_degree=3, active_sh_degree=3), means.cpu())
