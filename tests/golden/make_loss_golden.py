#!/usr/bin/env python
"""Writes tests/golden/photometric_loss.npz: l1_loss, ssim and the training loss's gradient computed by the REFERENCE's own
gaussian-splatting/utils/loss_utils.py, loaded unmodified from its path and run on CPU torch, for tests/test_loss_ref.py and
tests/test_photometric_loss_hip.py.

Per case of tests/_loss_ref.py's GOLDEN_CASES: the float32 inputs a (img1) and b (img2); at float64 (inputs cast up, so the
reference's `window.type_as(img1)` makes the whole evaluation float64) l1, ssim and the autograd gradient with respect to img1 of
(1 - 0.2) l1 + 0.2 (1 - ssim), the loss of train.py:92; for the 4-D case also ssim(size_average=False); at float32 the same two
scalars, as the reference runs.  Build container only (needs the reference tree); only data is committed.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = "/root/reference/third_party/PhysGaussian/gaussian-splatting/utils/loss_utils.py"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _loss_ref as lr  # noqa: E402

LAMBDA = 0.2


def main():
    spec = importlib.util.spec_from_file_location("reference_loss_utils", REF)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {"cases": np.array(lr.GOLDEN_CASES), "lambda_dssim": np.float64(LAMBDA)}
    for name in lr.GOLDEN_CASES:
        a, b = lr.make_case(name)
        out[f"{name}.a"], out[f"{name}.b"] = a, b
        for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
            ta = torch.from_numpy(a).to(dt).requires_grad_(True)
            tb = torch.from_numpy(b).to(dt)
            l1, ss = ref.l1_loss(ta, tb), ref.ssim(ta, tb)
            out[f"{name}.l1_{tag}"], out[f"{name}.ssim_{tag}"] = l1.detach().numpy(), ss.detach().numpy()
            if tag == "f64":
                loss = (1.0 - LAMBDA) * l1 + LAMBDA * (1.0 - ss)
                out[f"{name}.grad_f64"] = torch.autograd.grad(loss, ta)[0].numpy()
                if ta.dim() == 4:
                    out[f"{name}.ssim_per_image_f64"] = ref.ssim(ta, tb, size_average=False).detach().numpy()
    path = os.path.join(HERE, "photometric_loss.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
