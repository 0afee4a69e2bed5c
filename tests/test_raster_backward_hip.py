"""GPU tests of the rasteriser's backward pass (pixie_raster_backward behind torch autograd, pixie_amd/rasterizer.py) against the torch
oracle tests/_raster_grad_ref.py.

Bar, per case and quantity q (rel-L2 over all Gaussians): let y_q be the oracle's own float32-against-float64 distance; the HIP
gradient must lie within 3 y_q + 2 K 2^-24 of the float64 gradient, K being the scene's largest n_contrib (the module docstring of
tests/test_raster_grad_math.py derives the two terms).  Gradients of culled Gaussians are exactly zero.  With -s the ratios and
yardsticks are printed and written to profiles/raster_backward_parity.txt."""
import os

import numpy as np
import pytest
import torch

from tests import _raster_grad_ref as gr

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINES = []


@pytest.fixture(scope="module", autouse=True)
def parity_file(request):
    yield
    if request.config.getoption("capture") == "no" and LINES:
        name = torch.cuda.get_device_name(0) if torch.cuda.is_available() else "no device"
        with open(os.path.join(REPO, "profiles", "raster_backward_parity.txt"), "w") as f:
            f.write("Backward pass of the rasteriser against the float64 torch oracle (tests/test_raster_backward_hip.py -s)\n")
            f.write(f"device: {name}; torch {torch.__version__}\n")
            f.write("rel-L2 per quantity over all Gaussians; y = the oracle's float32 run against its float64 run; bar = 3 y + 2 K 2^-24\n\n")
            f.write("\n".join(LINES) + "\n")


def settings_of(s, dev, sh_degree=0):
    from pixie_amd.rasterizer import GaussianRasterizationSettings
    cam = s["cam"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return GaussianRasterizationSettings(image_height=cam["H"], image_width=cam["W"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                                         bg=t(s["bg"]), scale_modifier=s["scale_modifier"], viewmatrix=t(cam["V"]), projmatrix=t(cam["P"]),
                                         sh_degree=sh_degree, campos=t(cam["campos"]), prefiltered=False, debug=False)


def leaves_of(s, kw, dev, requires=None):
    """the rasteriser's keyword inputs as leaf tensors; `requires`: the names that require grad (default: all)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    x = dict(means3D=t(s["means"]), opacities=t(np.asarray(s["opacity"]).reshape(-1, 1)))
    x["means2D"] = torch.zeros_like(x["means3D"])
    if "cov6" in kw:
        x["cov3D_precomp"] = t(kw["cov6"])
    else:
        x["scales"], x["rotations"] = t(s["scales"]), t(s["rotations"])
    if "shs" in kw:
        x["shs"] = t(kw["shs"])
    else:
        x["colors_precomp"] = t(s["colors"])
    for k, v in x.items():
        v.requires_grad_(requires is None or k in requires)
    return x


NAMES = dict(means3D="means3D", means2D="means2D", opacities="opacities", cov3D="cov3D_precomp", scales="scales", rotations="rotations",
             colors="colors_precomp", shs="shs")


def forward(r, x):
    return r(x["means3D"], x["means2D"], x["opacities"], **{k: v for k, v in x.items() if k not in ("means3D", "means2D", "opacities")})


def grads_of(x):
    return {q: (None if x[k].grad is None else x[k].grad.detach().cpu().numpy().astype(np.float64)) for q, k in NAMES.items() if k in x}


def hip_grads(dev, s, kw, w, r=None):
    from pixie_amd.rasterizer import GaussianRasterizer
    r = r or GaussianRasterizer(settings_of(s, dev, kw.get("sh_degree", 0)))
    x = leaves_of(s, kw, dev)
    color, radii = forward(r, x)
    (color * torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(dev)).sum().backward()
    return grads_of(x), color.detach(), radii


def check(tag, got, ref):
    s, kw, w, share, r64, y = ref
    assert share <= gr.MAX_ZERO_SHARE, f"{tag}: {share:.4f} of the pixels are zero-weighted: the scene is not fit to compare on"
    K = r64["n_contrib_max"]
    culled = ~r64["valid"]
    for q, want in r64["grads"].items():
        g = got[q]
        assert g is not None and np.isfinite(g).all(), f"{tag} {q}"
        g = g.reshape(want.shape)
        assert np.all(g[culled] == 0), f"{tag} {q}: a culled Gaussian has a gradient"
        err = gr.rel_l2(g, want)
        line = f"{tag}: {q}: y {y[q]:.3e}, HIP error {err:.3e} = {err / y[q] if y[q] > 0 else 0.0:.2f} y, K {K}, bar {gr.bar(y[q], K):.3e}"
        print(line)
        LINES.append(line)
        assert err <= gr.bar(y[q], K), f"{tag} {q}: error {err:.3e} exceeds 3 y + 2 K 2^-24 = {gr.bar(y[q], K):.3e}"
    m2 = got["means2D"]
    assert m2.shape == (len(s["means"]), 3) and np.all(m2[:, 2] == 0)


CASES = [(n, "cov", None) for n in ("e", "d", "i", "g", "f", "h", "w")] + [(n, "sr", 3) for n in ("d", "i", "w")] + [("w", "sr", k) for k in (0, 1, 2)]


@pytest.mark.parametrize("name,form,degree", CASES)
def test_gradients_against_the_oracle(hip_device, name, form, degree):
    ref = gr.reference(name, form, degree)
    s, kw, w, share, r64, y = ref
    got, color, radii = hip_grads(hip_device, s, kw, w)
    check(f"scene {name} {form} sh {degree}", got, ref)
    if name in ("f", "h"):
        assert all(np.all(g == 0) for g in got.values())
    if name == "w":
        contributes = np.abs(r64["grads"]["opacities"]) > 0
        assert (r64["clamped"] & contributes).any(), "the 1.3 tanfov clamp is active on no contributing Gaussian"
        assert len(s["means"]) <= 2500 and s["cam"]["W"] <= 128 and s["cam"]["H"] <= 128
    if name == "i":
        assert r64["n_contrib_max"] > 2 * 256          # several LDS batches walked


def test_backward_is_reproducible_bit_for_bit(hip_device):
    s, kw, w, *_ = gr.reference("i", "sr", 3)
    a, _, _ = hip_grads(hip_device, s, kw, w)
    b, _, _ = hip_grads(hip_device, s, kw, w)
    for q in a:
        assert np.array_equal(a[q], b[q]), q


def test_image_equals_the_no_grad_image(hip_device):
    from pixie_amd.rasterizer import GaussianRasterizer
    for name, form, degree in (("d", "cov", None), ("w", "sr", 3)):
        s, kw, w, *_ = gr.reference(name, form, degree)
        r = GaussianRasterizer(settings_of(s, hip_device, kw.get("sh_degree", 0)))
        x = leaves_of(s, kw, hip_device)
        color, radii = forward(r, x)
        assert color.requires_grad and not radii.requires_grad
        with torch.no_grad():
            plain, plain_radii = forward(r, x)
        assert not plain.requires_grad
        assert torch.equal(color.detach(), plain) and torch.equal(radii, plain_radii)


def test_two_forwards_then_their_backwards_in_reverse_order(hip_device):
    from pixie_amd.rasterizer import GaussianRasterizer
    ref_a, ref_b = gr.reference("d", "cov", None), gr.reference("d", "sr", 3)
    r = GaussianRasterizer(settings_of(ref_a[0], hip_device, 3))
    xa, xb = leaves_of(ref_a[0], ref_a[1], hip_device), leaves_of(ref_b[0], ref_b[1], hip_device)
    wt = lambda w: torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(hip_device)
    ca, _ = forward(r, xa)
    cb, _ = forward(r, xb)
    with torch.no_grad():
        forward(r, xa)                                   # and the module's shared workspace is overwritten as well
    (cb * wt(ref_b[2])).sum().backward()
    (ca * wt(ref_a[2])).sum().backward()
    check("interleaved, first forward (d cov)", grads_of(xa), ref_a)
    check("interleaved, second forward (d sr sh 3)", grads_of(xb), ref_b)


def test_first_call_beyond_the_first_guess_regrows(hip_device):
    from pixie_amd.rasterizer import GaussianRasterizer
    ref = gr.reference("e", "cov", None)
    s, kw, w, *_ = ref
    r = GaussianRasterizer(settings_of(s, hip_device))
    got, color, radii = hip_grads(hip_device, s, kw, w, r=r)
    count = r.last_instances
    assert count > 4 * len(s["means"]) and r._owned_hint[1] == count + count // 2      # the 4 n guess was too small: grown once
    assert r._workspace is None                          # the module's shared workspace was not involved
    check("regrow (e cov)", got, ref)
    with torch.no_grad():
        plain, _ = forward(r, leaves_of(s, kw, hip_device))
    assert torch.equal(plain, color)


def test_only_what_requires_grad_gets_a_gradient(hip_device):
    from pixie_amd.rasterizer import GaussianRasterizer
    ref = gr.reference("d", "cov", None)
    s, kw, w, share, r64, y = ref
    x = leaves_of(s, kw, hip_device, requires=("opacities",))
    color, _ = forward(GaussianRasterizer(settings_of(s, hip_device)), x)
    (color * torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(hip_device)).sum().backward()
    for k, v in x.items():
        assert (v.grad is not None) == (k == "opacities"), k
    assert x["opacities"].grad.shape == x["opacities"].shape
    err = gr.rel_l2(x["opacities"].grad.cpu().numpy().reshape(-1), r64["grads"]["opacities"])
    assert err <= gr.bar(y["opacities"], r64["n_contrib_max"])


def test_means2d_receives_the_screen_space_gradient(hip_device):
    from pixie_amd.rasterizer import GaussianRasterizer
    ref = gr.reference("d", "cov", None)
    s, kw, w, share, r64, y = ref
    x = leaves_of(s, kw, hip_device)
    means2D = torch.zeros_like(x["means3D"], requires_grad=True)            # as train.py makes its screenspace_points
    means2D.retain_grad()
    x["means2D"] = means2D
    color, _ = forward(GaussianRasterizer(settings_of(s, hip_device)), x)
    (color * torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(hip_device)).sum().backward()
    g = means2D.grad
    assert g is not None and g.shape == (len(s["means"]), 3) and bool((g[:, 2] == 0).all())
    assert gr.rel_l2(g.cpu().numpy(), r64["grads"]["means2D"]) <= gr.bar(y["means2D"], r64["n_contrib_max"])


def test_render_is_differentiable(hip_device):
    """fails on a forward-only rasteriser: the colour carries a graph and loss.backward() fills .grad"""
    from pixie_amd.rasterizer import GaussianRasterizer
    s, kw, w, share = gr.case("small", "sr", 3)
    x = leaves_of(s, kw, hip_device)
    out, radii = forward(GaussianRasterizer(settings_of(s, hip_device, 3)), x)
    assert out.requires_grad and not radii.requires_grad
    out.square().mean().backward()
    for k, v in x.items():
        assert v.grad is not None and v.grad.shape == v.shape and bool(torch.isfinite(v.grad).all()), k
    assert all(float(x[k].grad.abs().max()) > 0 for k in ("means3D", "opacities", "scales", "rotations", "shs", "means2D"))


def test_adam_moves_a_render_towards_a_target(hip_device):
    """300 Gaussians at 64 x 64, scales / rotations + SH: 50 Adam steps towards an image rendered from perturbed parameters"""
    from pixie_amd.rasterizer import GaussianRasterizer
    from tests import _raster_ref as rr
    rng = np.random.default_rng(17)
    s = rr._cloud(rng, 300, (0, 0, 0), (0.5, 0.5, 0.5), 0.04, 0.15)
    s["cam"], s["bg"], s["scale_modifier"] = rr.look_at_camera((0.0, 0.0, -3.0), (0, 0, 0), 45.0, 64, 64), np.array([0.1, 0.2, 0.3], np.float32), 1.0
    shs = (rng.normal(size=(300, 16, 3)) * 0.2).astype(np.float32)
    shs[:, 0] += 1.0
    r = GaussianRasterizer(settings_of(s, hip_device, 3))
    target_x = leaves_of(s, dict(shs=shs), hip_device, requires=())
    with torch.no_grad():
        target, _ = forward(r, target_x)
    gen = torch.Generator(device="cpu").manual_seed(3)
    noise = {"means3D": 0.03, "opacities": 0.1, "scales": 0.01, "rotations": 0.05, "shs": 0.1}
    x = {k: (v.detach() + (torch.randn(v.shape, generator=gen) * noise[k]).to(hip_device) if k in noise else v.detach()) for k, v in target_x.items()}
    x["opacities"] = x["opacities"].clamp(0.02, 1.0)
    x["scales"] = x["scales"].clamp_min(0.005)
    params = [x[k].requires_grad_(True) for k in noise]
    opt = torch.optim.Adam(params, lr=2e-3)
    losses = []
    for _ in range(50):
        opt.zero_grad()
        color, _ = forward(r, x)
        loss = (color - target).abs().mean()
        loss.backward()
        opt.step()
        with torch.no_grad():
            x["opacities"].clamp_(0.02, 1.0)
            x["scales"].clamp_min_(0.005)
        losses.append(float(loss.detach()))
    assert all(bool(torch.isfinite(p).all()) for p in params)
    print(f"Adam: L1 {losses[0]:.5f} -> {losses[-1]:.5f}")
    assert losses[-1] < losses[0]
