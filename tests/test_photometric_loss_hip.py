"""GPU checks of the fused photometric loss (pixie_amd/losses.py, pixie_amd/csrc/photometric.hip) against tests/_loss_ref.py, whose
float64 run tests/test_loss_ref.py pins to the reference's own numbers.

Bars, in the project's yardstick form.  Let y be the distance of the float32 restatement (the reference's expression as torch
float32 ops, evaluated on the CPU) from the float64 one: the absolute difference for a scalar, the relative L2 for the gradient.
The HIP value must lie within 3 y + 4 * 2^-24 of float64 for l1 and ssim (the values are O(1); half an ulp of a float32 result is
2^-25), and within 3 y + 2 * 121 * 2^-24 of float64 for the gradient (a 121-term tap sum carries up to 121 u).  Where the
gradient is exactly zero (a == b) a relative error has no meaning: there l1 = 0 exactly, ssim = 1 within its bar, and the gradient
must be finite (its size is printed).
The ratios are printed (-s); profiles/photometric_loss_parity.txt is that output of a run on an MI355X."""
import os

import numpy as np
import pytest
import torch

from tests import _loss_ref as lr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photometric_loss.npz")
LAMBDA = 0.2
_cache = {}


def reference(name):
    """float64 and float32 restatements, computed once per case on the CPU: scalars, the training loss's gradient, per-image SSIM"""
    if name in _cache:
        return _cache[name]
    a, b = lr.make_case(name)
    out = {"a": a, "b": b}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        ta, tb = torch.from_numpy(a).to(dt).requires_grad_(True), torch.from_numpy(b).to(dt)
        l1, ss = lr.l1_loss(ta, tb), lr.ssim(ta, tb)
        g = torch.autograd.grad((1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - ss), ta)[0]
        out["l1" + tag], out["ssim" + tag], out["grad" + tag] = float(l1.detach()), float(ss.detach()), g.double()
        if ta.dim() == 4:
            out["per" + tag] = lr.ssim(ta.detach(), tb, size_average=False).double()
    _cache[name] = out
    return out


def measure(name, dev):
    """the fused loss on the device: l1, ssim, the gradient of the training loss"""
    from pixie_amd.losses import photometric_terms
    r = reference(name)
    ta = torch.from_numpy(r["a"]).to(dev).requires_grad_(True)
    tb = torch.from_numpy(r["b"]).to(dev)
    l1, ss = photometric_terms(ta, tb)
    ((1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - ss)).backward()
    return float(l1.detach()), float(ss.detach()), ta.grad.detach().cpu().double()


def figures(name, dev):
    """per quantity: (error of the HIP value against float64, yardstick y, bar)"""
    r = reference(name)
    l1, ss, g = measure(name, dev)
    out = {}
    for key, got in (("l1", l1), ("ssim", ss)):
        y = abs(r[key + "32"] - r[key + "64"])
        out[key] = (abs(got - r[key + "64"]), y, 3 * y + 4 * U)
    if not np.array_equal(r["a"], r["b"]):
        y = lr.rel_l2(r["grad32"], r["grad64"])
        out["grad"] = (lr.rel_l2(g, r["grad64"]), y, 3 * y + 2 * 121 * U)
    else:                             # a == b: the gradient is exactly zero, so a relative error has no meaning; it must be finite
        n = r["grad64"].numel()
        print(f"{name}: gradient where it is exactly zero, rms in units of 1 / N: HIP {float(torch.linalg.norm(g)) * np.sqrt(n):.2e}, "
              f"float32 restatement {float(torch.linalg.norm(r['grad32'])) * np.sqrt(n):.2e}")
    assert bool(torch.isfinite(g).all())
    return out


def report(name, fig):
    return f"{name}: " + ", ".join(f"{k} err {e:.2e} y {y:.2e} bar {bar:.2e} (err / y {(f'{e / y:.2f}') if y > 0 else 'n/a'})" for k, (e, y, bar) in fig.items())


@pytest.mark.parametrize("name", lr.CASES)
def test_values_and_gradient_within_the_yardstick_bars(hip_device, name):
    fig = figures(name, hip_device)
    print(report(name, fig))
    for key, (err, y, bar) in fig.items():
        assert err <= bar, (name, key, err, y, bar)
    if name == "equal":
        l1, ss, _ = measure(name, hip_device)
        assert l1 == 0.0 and abs(ss - 1.0) <= 4 * U


def test_size_average_false_returns_per_image_means(hip_device):
    from pixie_amd.losses import ssim
    r = reference("batch")
    ta, tb = torch.from_numpy(r["a"]).to(hip_device), torch.from_numpy(r["b"]).to(hip_device)
    per = ssim(ta, tb, size_average=False)
    assert per.shape == (2,)
    y = float((r["per32"] - r["per64"]).abs().max())
    err = float((per.cpu().double() - r["per64"]).abs().max())
    print(f"batch, per image: err {err:.2e} y {y:.2e}")
    assert err <= 3 * y + 4 * U
    with pytest.raises(ValueError, match="size_average"):
        ssim(ta[0], tb[0], size_average=False)
    # each image's gradient is its own: weight the two images differently
    ta.requires_grad_(True)
    w = torch.tensor([1.0, -2.0], device=hip_device)
    (ssim(ta, tb, size_average=False) * w).sum().backward()
    a64 = torch.from_numpy(r["a"]).double().requires_grad_(True)
    (lr.ssim(a64, torch.from_numpy(r["b"]).double(), size_average=False) * w.cpu().double()).sum().backward()
    a32 = torch.from_numpy(r["a"]).requires_grad_(True)
    (lr.ssim(a32, torch.from_numpy(r["b"]), size_average=False) * w.cpu()).sum().backward()
    y = lr.rel_l2(a32.grad, a64.grad)
    assert lr.rel_l2(ta.grad.cpu(), a64.grad) <= 3 * y + 2 * 121 * U


@pytest.mark.parametrize("name", lr.GOLDEN_CASES)
def test_golden_inputs_reproduce_the_reference_numbers(hip_device, name):
    """the reference's own float64 numbers (tests/golden/photometric_loss.npz), within the same bars"""
    g = np.load(GOLDEN)
    r = reference(name)
    assert np.array_equal(r["a"], g[f"{name}.a"]) and np.array_equal(r["b"], g[f"{name}.b"])
    l1, ss, grad = measure(name, hip_device)
    assert abs(l1 - float(g[f"{name}.l1_f64"])) <= 3 * abs(r["l132"] - r["l164"]) + 4 * U
    assert abs(ss - float(g[f"{name}.ssim_f64"])) <= 3 * abs(r["ssim32"] - r["ssim64"]) + 4 * U
    ref = torch.from_numpy(g[f"{name}.grad_f64"]).double()
    assert lr.rel_l2(grad, ref) <= 3 * lr.rel_l2(r["grad32"], r["grad64"]) + 2 * 121 * U


def test_two_runs_are_bit_equal(hip_device):
    for name in ("noise", "batch"):
        a, b = measure(name, hip_device), measure(name, hip_device)
        assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2])


def test_wrappers_agree_with_the_terms(hip_device):
    from pixie_amd.losses import l1_loss, photometric_loss, photometric_terms, ssim
    r = reference("noise")
    ta, tb = torch.from_numpy(r["a"]).to(hip_device), torch.from_numpy(r["b"]).to(hip_device)
    l1, ss = photometric_terms(ta, tb)
    assert l1.shape == () and ss.shape == ()
    assert torch.equal(l1_loss(ta, tb), l1) and torch.equal(ssim(ta, tb), ss)
    for lam in (0.2, 0.5):
        assert torch.equal(photometric_loss(ta, tb, lam), (1.0 - lam) * l1 + lam * (1.0 - ss))
    # 3-D and 4-D forms of one image are the same computation
    l1b, ssb = photometric_terms(ta[None], tb[None])
    assert torch.equal(l1b, l1) and torch.equal(ssb, ss)


def test_no_grad_retains_nothing(hip_device):
    from pixie_amd.losses import photometric_loss, photometric_terms
    r = reference("noise")
    ta = torch.from_numpy(r["a"]).to(hip_device).requires_grad_(True)
    tb = torch.from_numpy(r["b"]).to(hip_device)
    with_grad = photometric_loss(ta, tb)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(hip_device)
    with torch.no_grad():
        out = photometric_loss(ta, tb)
    torch.cuda.synchronize()
    assert out.grad_fn is None and not out.requires_grad
    assert torch.cuda.memory_allocated(hip_device) - before <= 1024         # the scalar; no planes, no workspace
    assert torch.equal(out, with_grad.detach())
    l1, ss = photometric_terms(ta.detach(), tb)                               # an input that does not require grad: no graph either
    assert l1.grad_fn is None and ss.grad_fn is None


def test_argument_errors(hip_device):
    from pixie_amd.losses import l1_loss, photometric_loss, ssim
    a = torch.rand((3, 8, 8), device=hip_device)
    b = torch.rand((3, 8, 8), device=hip_device)
    with pytest.raises(ValueError, match="must not require grad"):
        photometric_loss(a, b.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="window_size"):
        ssim(a, b, window_size=7)
    with pytest.raises(ValueError, match="float32"):
        l1_loss(a.double(), b.double())
    with pytest.raises(ValueError, match="shapes differ"):
        l1_loss(a, b[:, :7])
    with pytest.raises(ValueError, match="HIP device"):
        l1_loss(a.cpu(), b.cpu())
    with pytest.raises(ValueError, match=r"\(C, H, W\)"):
        l1_loss(a[0], b[0])


def test_interleaved_forwards_keep_their_own_gradients(hip_device):
    from pixie_amd.losses import photometric_loss
    alone = {}
    for name in ("noise", "near"):
        alone[name] = measure(name, hip_device)[2]
    leaves, losses = {}, {}
    for name in ("noise", "near"):                       # both forwards first
        r = reference(name)
        leaves[name] = torch.from_numpy(r["a"]).to(hip_device).requires_grad_(True)
        losses[name] = photometric_loss(leaves[name], torch.from_numpy(r["b"]).to(hip_device), LAMBDA)
    for name in ("noise", "near"):                       # then the backwards, first forward first
        losses[name].backward()
    for name in ("noise", "near"):
        assert torch.equal(leaves[name].grad.cpu().double(), alone[name]), name


def test_non_contiguous_input_and_non_default_stream(hip_device):
    from pixie_amd.losses import photometric_terms
    r = reference("noise")
    ref = measure("noise", hip_device)
    hwc_a = torch.from_numpy(np.ascontiguousarray(r["a"].transpose(1, 2, 0))).to(hip_device)
    hwc_b = torch.from_numpy(np.ascontiguousarray(r["b"].transpose(1, 2, 0))).to(hip_device)
    stream = torch.cuda.Stream(device=hip_device)
    stream.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(stream):
        l1, ss = photometric_terms(hwc_a.permute(2, 0, 1), hwc_b.permute(2, 0, 1))
    stream.synchronize()
    assert float(l1) == ref[0] and float(ss) == ref[1]
