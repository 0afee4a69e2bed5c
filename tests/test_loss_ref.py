"""CPU checks that pin the formulas of the fused photometric loss before anything runs on a GPU: the torch restatement of
tests/_loss_ref.py equals the reference's own numbers (tests/golden/photometric_loss.npz, written by
tests/golden/make_loss_golden.py from gaussian-splatting/utils/loss_utils.py) in float64 to 1e-12, and the closed-form backward that
pixie_amd/csrc/photometric.hip implements equals autograd in float64 to 1e-12 relative L2."""
import os

import numpy as np
import pytest
import torch

from tests import _loss_ref as lr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photometric_loss.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def t64(x):
    return torch.from_numpy(np.asarray(x)).double()


@pytest.mark.parametrize("name", lr.GOLDEN_CASES)
def test_restatement_equals_the_reference(golden, name):
    a, b = lr.make_case(name)
    assert np.array_equal(a, golden[f"{name}.a"]) and np.array_equal(b, golden[f"{name}.b"]), "the case generator drifted from the golden"
    ta, tb = t64(a).requires_grad_(True), t64(b)
    l1, ss = lr.l1_loss(ta, tb), lr.ssim(ta, tb)
    assert abs(float(l1.detach()) - float(golden[f"{name}.l1_f64"])) <= 1e-12
    assert abs(float(ss.detach()) - float(golden[f"{name}.ssim_f64"])) <= 1e-12
    lam = float(golden["lambda_dssim"])
    g = torch.autograd.grad(lr.photometric_loss(ta, tb, lam), ta)[0]
    assert lr.rel_l2(g, t64(golden[f"{name}.grad_f64"])) <= 1e-12
    if ta.dim() == 4:
        per = lr.ssim(ta, tb, size_average=False)
        assert torch.max(torch.abs(per - t64(golden[f"{name}.ssim_per_image_f64"]))) <= 1e-12
        l1_i, ss_i = lr.per_image_terms(ta, tb)
        assert torch.max(torch.abs(ss_i - per)) <= 1e-15 and abs(float(l1_i.mean().detach()) - float(l1.detach())) <= 1e-15
    # the reference's own float32 run is the scale of what float32 can give
    print(f"{name}: reference float32 run off its float64 run by l1 {abs(float(golden[f'{name}.l1_f32']) - float(golden[f'{name}.l1_f64'])):.1e}, "
          f"ssim {abs(float(golden[f'{name}.ssim_f32']) - float(golden[f'{name}.ssim_f64'])):.1e}")


@pytest.mark.parametrize("name", lr.CASES)
def test_closed_form_backward_equals_autograd(name):
    a, b = lr.make_case(name)
    ta, tb = t64(a).requires_grad_(True), t64(b)
    bsz = ta.shape[0] if ta.dim() == 4 else 1
    gen = torch.Generator().manual_seed(3)
    g_l1, g_ss = torch.randn(bsz, generator=gen).double(), torch.randn(bsz, generator=gen).double()
    l1_i, ss_i = lr.per_image_terms(ta, tb)
    auto = torch.autograd.grad((g_l1 * l1_i).sum() + (g_ss * ss_i).sum(), ta)[0]
    closed = lr.closed_form_grad(ta.detach(), tb, g_l1, g_ss)
    assert closed.shape == auto.shape
    if name == "equal":               # a == b: SSIM is at its maximum and sign(0) = 0, so the gradient is zero and only an absolute bar has meaning
        assert float(auto.abs().max()) <= 1e-15 and float(closed.abs().max()) <= 1e-15
        return
    assert lr.rel_l2(closed, auto) <= 1e-12
    # each term on its own as well: a wrong SSIM term must not hide behind the larger L1 term
    zero = torch.zeros(bsz, dtype=torch.float64)
    auto_ss = torch.autograd.grad((g_ss * lr.per_image_terms(ta, tb)[1]).sum(), ta)[0]
    assert lr.rel_l2(lr.closed_form_grad(ta.detach(), tb, zero, g_ss), auto_ss) <= 1e-12


def test_sign_of_zero_and_the_borders_are_exercised():
    a, b = lr.make_case("flat_edges")
    assert (a == b).any() and (a != b).any()
    ta, tb = t64(a), t64(b)
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    g = lr.closed_form_grad(ta, tb, one, zero)
    assert torch.all(g[ta == tb] == 0.0) and torch.all(g[ta != tb] != 0.0)          # sign(0) = 0, as torch.abs has it
    # zero padding: the window hangs over the border, so SSIM of a constant image pair falls off there
    c = torch.full((1, 24, 24), 0.5, dtype=torch.float64)
    m = lr.ssim_map(c, c * 0.5)[0, 0]
    assert abs(float(m[12, 12]) - float(m[11, 13])) < 1e-15 and abs(float(m[0, 0]) - float(m[12, 12])) > 1e-3
    # an image smaller than the window and a single pixel are all border
    for name in ("small", "pixel"):
        a, b = lr.make_case(name)
        assert torch.isfinite(lr.ssim(t64(a), t64(b)))


def test_float32_restatement_is_close_to_float64():
    for name in lr.CASES:
        a, b = lr.make_case(name)
        s32 = float(lr.ssim(torch.from_numpy(a), torch.from_numpy(b)))
        s64 = float(lr.ssim(t64(a), t64(b)))
        assert abs(s32 - s64) < 1e-4, (name, s32, s64)
