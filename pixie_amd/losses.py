"""The photometric loss of 3DGS training, fused: L1 and SSIM of a render against its ground truth in one pass, with a HIP backward.

Drop-ins for gaussian-splatting/utils/loss_utils.py as train.py:91-92 uses it:
  * `l1_loss(network_output, gt)` and `ssim(img1, img2, window_size=11, size_average=True)`: the reference's signatures;
  * `photometric_terms(image, gt) -> (l1, ssim)`: both from ONE forward (one fused launch and a finalise) and, with grad mode on and
    `image.requires_grad`, one backward launch for both;
  * `photometric_loss(image, gt, lambda_dssim=0.2) = (1 - lambda) l1 + lambda (1 - ssim)`, the expression of train.py:92.
Calling l1_loss and ssim separately runs the fused pass twice; train.py's two lines become one `photometric_loss` call.

Inputs are (C, H, W) or (B, C, H, W) float32 tensors on a HIP device, any C, H, W >= 1.  SSIM is the reference's: window 11,
sigma 1.5, zero padding 5, one window per channel, C1 = 1e-4, C2 = 9e-4; the window is applied separably, which differs from the
121-tap form at rounding level.  `size_average=False` takes a 4-D input and returns (B,).

The gradient is with respect to the first argument only; `gt` must not require grad.  The three planes the backward convolves
live in a workspace owned by the autograd node, so forwards and backwards may interleave freely.  Under torch.no_grad(), or when
`image` does not require grad, no planes are written and nothing is kept.  No double backward.  Sums are taken in a fixed order
without floating-point atomics: values and gradients are bit-identical from run to run.  The pass makes no host synchronise.
There is no CPU compute path: a host tensor is refused.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def _check_pair(image, gt, who):
    for t, what in ((image, "the first argument"), (gt, "the second argument")):
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise ValueError(f"{who}: {what} must be a tensor on a HIP device (there is no CPU path)")
        if t.dtype != torch.float32:
            raise ValueError(f"{who}: {what} must be float32, got {t.dtype}")
    if image.shape != gt.shape:
        raise ValueError(f"{who}: shapes differ: {tuple(image.shape)} and {tuple(gt.shape)}")
    if image.device != gt.device:
        raise ValueError(f"{who}: the two images are on different devices")
    if image.dim() not in (3, 4) or min(image.shape) < 1:
        raise ValueError(f"{who}: images must be (C, H, W) or (B, C, H, W) with every extent >= 1, got {tuple(image.shape)}")
    if gt.requires_grad:
        raise ValueError(f"{who}: the gradient is with respect to the first argument only; the second must not require grad")


def _forward(image, gt, with_grad):
    """image, gt: contiguous (B, C, H, W).  Returns (l1 (B,), ssim (B,), workspace)."""
    b, c, h, w = (int(s) for s in image.shape)
    lib = _lib.load()
    with torch.cuda.device(image.device):
        need = lib.pixie_photometric_workspace_bytes(b, c, h, w, int(with_grad))
        if need < 0:
            _lib.check(1, "pixie_photometric_workspace_bytes", lib=lib)
        ws = torch.empty((max(int(need), 16),), dtype=torch.uint8, device=image.device)
        l1 = torch.empty((b,), dtype=torch.float32, device=image.device)
        ss = torch.empty((b,), dtype=torch.float32, device=image.device)
        rc = lib.pixie_photometric_forward(C.c_void_p(image.data_ptr()), C.c_void_p(gt.data_ptr()), b, c, h, w, C.c_void_p(ws.data_ptr()),
                                           ws.numel(), int(with_grad), C.c_void_p(l1.data_ptr()), C.c_void_p(ss.data_ptr()),
                                           _lib.current_stream_ptr())
        _lib.check(rc, "pixie_photometric_forward", lib=lib)
    return l1, ss, ws


class _Photometric(torch.autograd.Function):
    """forward = pixie_photometric_forward with the gradient planes, on a workspace of its own; backward = one
    pixie_photometric_backward."""

    @staticmethod
    def forward(ctx, image, gt):
        l1, ss, ws = _forward(image, gt, True)
        ctx.save_for_backward(image, gt)
        ctx.workspace = ws
        return l1, ss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_l1, g_ssim):
        image, gt = ctx.saved_tensors
        b, c, h, w = (int(s) for s in image.shape)
        g_l1 = g_l1.to(torch.float32).contiguous()
        g_ssim = g_ssim.to(torch.float32).contiguous()
        grad = torch.empty_like(image)
        lib = _lib.load()
        with torch.cuda.device(image.device):
            rc = lib.pixie_photometric_backward(C.c_void_p(image.data_ptr()), C.c_void_p(gt.data_ptr()), b, c, h, w,
                                                C.c_void_p(ctx.workspace.data_ptr()), C.c_void_p(g_l1.data_ptr()),
                                                C.c_void_p(g_ssim.data_ptr()), C.c_void_p(grad.data_ptr()), _lib.current_stream_ptr())
            _lib.check(rc, "pixie_photometric_backward", lib=lib)
        return grad, None


def _terms_per_image(image, gt, who):
    """(l1 (B,), ssim (B,)) of a checked pair; B = 1 for 3-D input."""
    _check_pair(image, gt, who)
    image4 = (image if image.dim() == 4 else image.unsqueeze(0)).contiguous()
    gt4 = (gt if gt.dim() == 4 else gt.unsqueeze(0)).detach().contiguous()
    if torch.is_grad_enabled() and image.requires_grad:
        return _Photometric.apply(image4, gt4)
    l1, ss, _ = _forward(image4.detach(), gt4, False)
    return l1, ss


def _reduce(v, image):
    return v.reshape(()) if image.dim() == 3 or v.numel() == 1 else v.mean()


def photometric_terms(image, gt):
    """(l1, ssim), both scalars: the means over every element, as l1_loss and ssim(size_average=True) give them."""
    l1, ss = _terms_per_image(image, gt, "photometric_terms")
    return _reduce(l1, image), _reduce(ss, image)


def l1_loss(network_output, gt):
    return _reduce(_terms_per_image(network_output, gt, "l1_loss")[0], network_output)


def ssim(img1, img2, window_size=11, size_average=True):
    if window_size != 11:
        raise ValueError(f"ssim: the fused kernel is built for window_size 11, got {window_size}")
    ss = _terms_per_image(img1, img2, "ssim")[1]
    if size_average:
        return _reduce(ss, img1)
    if img1.dim() != 4:
        raise ValueError("ssim: size_average=False needs a (B, C, H, W) input")
    return ss


def photometric_loss(image, gt, lambda_dssim=0.2):
    """(1 - lambda_dssim) * l1 + lambda_dssim * (1 - ssim): the loss of train.py:92 from one fused forward."""
    l1, ss = photometric_terms(image, gt)
    return (1.0 - lambda_dssim) * l1 + lambda_dssim * (1.0 - ss)
