"""One 3DGS training loop on this library's natives alone: scales from distCUDA2 as create_from_pcd sets them, the differentiable
rasteriser, the fused photometric loss, Adam."""
import numpy as np
import pytest
import torch

from tests import _loss_ref as lr
from tests import _raster_ref as rr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def test_forty_adam_steps_on_the_training_natives(hip_device):
    from pixie_amd.losses import photometric_loss
    from pixie_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from pixie_amd.simple_knn import distCUDA2
    dev = hip_device
    rng = np.random.default_rng(23)
    n = 300
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    points = t(rng.uniform(-0.5, 0.5, size=(n, 3)))                       # the unit cube, centred on the camera's target
    dist2 = torch.clamp_min(distCUDA2(points), 0.0000001)                 # scene/gaussian_model.py:134-135
    log_scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
    assert bool(torch.isfinite(log_scales).all())
    cam = rr.look_at_camera((0.0, 0.0, -3.0), (0, 0, 0), 45.0, 64, 64)
    settings = GaussianRasterizationSettings(image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                             bg=t([0.1, 0.2, 0.3]), scale_modifier=1.0, viewmatrix=t(cam["V"]), projmatrix=t(cam["P"]),
                                             sh_degree=0, campos=t(cam["campos"]), prefiltered=False, debug=False)
    r = GaussianRasterizer(settings)
    truth = dict(means=points, log_scales=log_scales, rotations=t(np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))),
                 logit_opacity=t(rng.uniform(-1.0, 2.0, size=(n, 1))), colors=t(rng.uniform(0.0, 1.0, size=(n, 3))))

    def render(p):
        color, _ = r(means3D=p["means"], means2D=torch.zeros_like(p["means"]), opacities=torch.sigmoid(p["logit_opacity"]),
                     colors_precomp=p["colors"], scales=torch.exp(p["log_scales"]), rotations=p["rotations"])
        return color

    with torch.no_grad():
        target = render(truth)
    gen = torch.Generator(device="cpu").manual_seed(5)
    noise = dict(means=0.02, log_scales=0.1, rotations=0.05, logit_opacity=0.3, colors=0.15)
    params = {k: (v + (torch.randn(v.shape, generator=gen) * noise[k]).to(dev)).requires_grad_(True) for k, v in truth.items()}

    # step 0: the gradients through the fused loss against those through the float32 torch expression, at the image and below
    image = render(params)
    image.retain_grad()
    photometric_loss(image, target).backward()
    fused_image_grad = image.grad.detach().cpu()
    fused = {k: v.grad.detach().clone() for k, v in params.items()}
    for v in params.values():
        v.grad = None
    image = render(params)
    image.retain_grad()
    lr.photometric_loss(image, target).backward()
    a64 = image.detach().cpu().double().requires_grad_(True)
    lr.photometric_loss(a64, target.cpu().double()).backward()
    y = lr.rel_l2(image.grad.cpu(), a64.grad)
    err = lr.rel_l2(fused_image_grad, a64.grad)
    print(f"image gradient at step 0: fused err {err:.2e}, torch float32 expression y {y:.2e}")
    assert err <= 3 * y + 2 * 121 * U
    for k, v in params.items():
        assert bool(torch.isfinite(fused[k]).all()) and float(fused[k].abs().max()) > 0, k
        v.grad = None

    opt = torch.optim.Adam(list(params.values()), lr=2e-3)
    losses = []
    for _ in range(40):
        opt.zero_grad()
        loss = photometric_loss(render(params), target)
        loss.backward()
        assert all(bool(torch.isfinite(v.grad).all()) for v in params.values())
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    print(f"Adam on (1 - 0.2) L1 + 0.2 (1 - SSIM): {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
