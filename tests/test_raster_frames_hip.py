"""GPU test of the frame hand-off: a jelly scene of pixie_amd/synthetic.py goes through SceneBatch.run_frames for 3 frames, and
rasterizer.render_frames turns what that returns into images -- bit for bit the per-frame GaussianRasterizer calls, frame 0 within
the bars of tests/test_raster_hip.py against the NumPy helper on a sample of tiles, later frames different (the scene moves) -- and
save_frame_png writes a frame the way the reference's frame loop does."""
import numpy as np
import pytest
import torch

from tests import _raster_ref as rr
from tests.test_mpm_batch_hip import make

pytestmark = pytest.mark.gpu


def test_render_frames_of_a_jelly_scene(hip_device, tmp_path):
    from pixie_amd.mpm_solver import FrameSchedule, SceneBatch
    from pixie_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, render_frames, save_frame_png
    from pixie_amd.synthetic import mpm_ball_scene
    n = 5000
    sc = mpm_ball_scene(n, seed=1, n_grid=32, scenario="tree")
    solver = make(sc)
    with SceneBatch([solver]) as sb:
        frames = sb.run_frames([FrameSchedule(1e-4, 60, 3, gs_num=n)])[0]
    pos, cov = frames[0], frames[1]
    assert pos.shape == (3, n, 3) and cov.shape == (3, n, 6)

    cam = rr.look_at_camera((0.0, -2.4, 0.3), (0.0, 0.0, 0.0), 40.0, 168, 120, up=(0.0, 0.0, -1.0))   # the export centres the ball at the origin
    rng = np.random.default_rng(2)
    opacity = rng.uniform(0.2, 1.0, n).astype(np.float32)
    colors = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    bg = np.array([1.0, 1.0, 1.0], np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(hip_device)
    settings = GaussianRasterizationSettings(image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=t(bg),
                                             scale_modifier=1.0, viewmatrix=t(cam["V"]), projmatrix=t(cam["P"]), sh_degree=0,
                                             campos=t(cam["campos"]), prefiltered=False, debug=False)
    images = render_frames(frames, settings, t(opacity), colors_precomp=t(colors))
    assert images.shape == (3, 3, cam["H"], cam["W"]) and images.device == hip_device and torch.isfinite(images).all()
    for f in range(3):
        single, radii = GaussianRasterizer(settings)(pos[f], None, t(opacity), colors_precomp=t(colors), cov3D_precomp=cov[f])
        assert torch.equal(images[f], single), f"frame {f}"
        assert (radii > 0).sum() > 0.9 * n
    assert not torch.equal(images[1], images[0]) and not torch.equal(images[2], images[0])      # the scene moves

    # frame 0 against the helper on a sample of tiles
    s = dict(means=pos[0].cpu().numpy(), opacity=opacity, colors=colors, cam=cam, bg=bg, scale_modifier=1.0)
    mask = np.random.default_rng(7).random(((cam["H"] + 15) // 16, (cam["W"] + 15) // 16)) < 0.25
    r64, r32, y = rr.yardstick(s, cov6=cov[0].cpu().numpy(), tile_mask=mask)
    keep = r64["selected"] & ~r64["borderline_pixels"]
    err = float(np.max(np.abs(images[0].cpu().numpy().astype(np.float64) - r64["color"])[:, keep]))
    print(f"jelly frame 0: {int(keep.sum())} pixels compared, y {y:.3e}, HIP error {err:.3e} = {err / y:.2f} y")
    assert r64["borderline_pixels"].sum() <= 0.005 * r64["selected"].sum()
    assert 0 < y <= rr.Y_CAP and err <= 3 * y

    # unselected Gaussians ride along with every frame (gs_simulation.py:602-606)
    m = 300
    extra = (t(rng.normal(size=(m, 3)).astype(np.float32) * 0.2), t(np.tile(np.array([[4e-4, 0, 0, 4e-4, 0, 4e-4]], np.float32), (m, 1))))
    op2, col2 = t(np.concatenate([opacity, np.full(m, 0.7, np.float32)])), t(np.concatenate([colors, np.zeros((m, 3), np.float32)]))
    with_extra = render_frames(frames, [settings] * 3, op2, colors_precomp=col2, unselected=extra)
    one, _ = GaussianRasterizer(settings)(torch.cat([pos[1], extra[0]]), None, op2, colors_precomp=col2, cov3D_precomp=torch.cat([cov[1], extra[1]]))
    assert torch.equal(with_extra[1], one) and not torch.equal(with_extra[1], images[1])

    try:
        from PIL import Image
    except ImportError:
        return                                   # the round trip needs Pillow; save_frame_png's own error is its message
    path = save_frame_png(str(tmp_path / "00000.png"), images[0])
    back = np.asarray(Image.open(path).convert("RGB"))
    want = np.round(np.clip(255.0 * images[0].cpu().numpy().astype(np.float32), 0, 255)).astype(np.uint8).transpose(1, 2, 0)
    assert back.shape == (cam["H"], cam["W"], 3) and np.array_equal(back, want)
