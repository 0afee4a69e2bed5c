"""distCUDA2: the one entry point gaussian-splatting uses of its `simple-knn` submodule.

Drop-in for `from simple_knn._C import distCUDA2` (scene/gaussian_model.py:20): `create_from_pcd` (:134) initialises every
Gaussian's scale from `log(sqrt(clamp_min(distCUDA2(points), 1e-7)))`.

    distCUDA2(points (N, 3) float32 on a HIP device) -> (N,) float32

out[i] is the mean of the three smallest squared distances from point i to the OTHER points (by index: a coincident point counts
at distance 0), in float32 as ((dx dx + dy dy) + dz dz) and ((b0 + b1) + b2) / 3 without fused multiply-adds.  One
pixie_knn_mean_dist2 call (HIP, pixie_amd/csrc/knn.hip) on the tensor's device and torch's current stream; no synchronise.  The
search is exact, so the result equals a float32 brute force in that expression order bit for bit, is the same from run to run, and
does not depend on the order of the rows.  A missing neighbour counts as FLT_MAX, as in the reference: one or two points give
+inf, three give FLT_MAX / 3.

The coordinates must be finite: a NaN leaves the affected points' values unspecified.  At most 2^24 points per call.
Difference from the reference: a CUDA build may contract the squared distance into fused multiply-adds, which moves a distance by
up to one ulp.  There is no CPU compute path: a host tensor is refused.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

MAX_POINTS = 1 << 24


def distCUDA2(points):
    if not torch.is_tensor(points) or points.device.type != "cuda":
        raise ValueError("distCUDA2: points must be a tensor on a HIP device (there is no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"distCUDA2: points must be (N, 3), got {tuple(points.shape)}")
    if points.dtype != torch.float32:
        raise ValueError(f"distCUDA2: points must be float32, got {points.dtype}")
    n = int(points.shape[0])
    if n > MAX_POINTS:
        raise ValueError(f"distCUDA2: {n} points exceed the 2^24 one call takes")
    pts = points.detach().contiguous()
    out = torch.empty((n,), dtype=torch.float32, device=pts.device)
    if n == 0:
        return out
    lib = _lib.load()
    with torch.cuda.device(pts.device):
        need = lib.pixie_knn_mean_dist2_scratch_bytes(n)
        if need < 0:
            _lib.check(1, "pixie_knn_mean_dist2_scratch_bytes", lib=lib)
        scratch = torch.empty((max(int(need), 16),), dtype=torch.uint8, device=pts.device)
        rc = lib.pixie_knn_mean_dist2(C.c_void_p(pts.data_ptr()), n, C.c_void_p(scratch.data_ptr()), scratch.numel(),
                                      C.c_void_p(out.data_ptr()), _lib.current_stream_ptr())
        _lib.check(rc, "pixie_knn_mean_dist2", lib=lib)
        # the scratch goes back to torch's caching allocator here; launches queued on this stream are ordered before any reuse
    return out
