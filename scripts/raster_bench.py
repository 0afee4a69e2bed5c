#!/usr/bin/env python
"""Times the forward rasteriser at the frame-export sizes of DESIGN 3.8: a ball of N Gaussians (the synthetic MPM scene's sizes) at
800 x 800.  HIP events around whole GaussianRasterizer calls (which include the one stream synchronise that reads the instance
count); per-launch times come from running this script under `rocprofv3 --kernel-trace --stats`.  Prints one line per size.

`--frames F` times a frame sequence instead: F frames of the ball (it drifts and swells a little from frame to frame) rendered by
`render_frames`, a call per frame, against one `render_frame_batch` call on the same tensors in the same process, the two
alternating `--reps` times after `--warmup` rounds of both.  Host clock around each, ending in a device synchronise.  Prints the
per-view instance counts, the group count, both times and whether the two image sequences are bit-equal.

`--backward` times the differentiable render instead: per size, the forward-only call (under no_grad, as above), then forward +
backward with means3D, opacities, colors_precomp and cov3D_precomp requiring grad and a fixed dL/dcolour, by HIP events around `--reps`
iterations after `--warmup`; it prints both next to the bytes of the backward's per-instance buffer (nine floats per instance) and
whether two backwards gave the same bits.  Per-kernel times come from running it under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixie_amd.rasterizer import (FrameBatchRasterizer, GaussianRasterizationSettings, GaussianRasterizer, render_frame_batch,  # noqa: E402
                                  render_frames)


def look_at_camera(eye, target, fovx_deg, W, H, up, znear=0.01, zfar=100.0):
    """row-vector view and full projection matrices of a pinhole camera (+z forward, y down), tan of the half fields of view"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    V = np.eye(4)
    V[:3, :3] = np.stack([right, np.cross(fwd, right), fwd], axis=1)
    V[3, :3] = -eye @ V[:3, :3]
    tanx = np.tan(np.radians(fovx_deg) / 2.0)
    tany = tanx * H / W
    Pm = np.zeros((4, 4))
    Pm[0, 0], Pm[1, 1], Pm[2, 2], Pm[3, 2], Pm[2, 3] = 1.0 / tanx, 1.0 / tany, zfar / (zfar - znear), -(zfar * znear) / (zfar - znear), 1.0
    return dict(V=V.astype(np.float32), P=(V @ Pm).astype(np.float32), tanfovx=float(tanx), tanfovy=float(tany), campos=eye.astype(np.float32))


def time_frames(a, n, st, pos, cov, opacity, colors):
    """F per-frame calls against one batched call on the same inputs; both rasterisers keep their workspace between rounds."""
    F = a.frames
    drift = torch.linspace(0.0, 0.05, F, device=pos.device)[:, None, None]
    frames = ((pos[None] * (1.0 + drift)).contiguous(), (cov[None] * (1.0 + drift) ** 2).contiguous())
    single, batch = GaussianRasterizer(st), FrameBatchRasterizer()
    out_loop = out_batch = None
    t_loop, t_batch = [], []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out_loop = render_frames(frames, st, opacity, colors_precomp=colors, rasterizer=single)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out_batch = render_frame_batch(frames, st, opacity, colors_precomp=colors, rasterizer=batch, out=out_batch)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep >= a.warmup:
            t_loop.append((t1 - t0) * 1e3)
            t_batch.append((t2 - t1) * 1e3)
    med = lambda v: float(np.median(v))
    print(json.dumps(dict(n=n, width=a.size, height=a.size, frames=F, reps=a.reps, per_frame_loop_ms=med(t_loop), batched_call_ms=med(t_batch),
                          per_frame_loop_ms_min_max=[min(t_loop), max(t_loop)], batched_call_ms_min_max=[min(t_batch), max(t_batch)],
                          batched_over_loop=med(t_batch) / med(t_loop), instances_per_view=batch.last_instances, groups=batch.last_groups,
                          workspace_bytes=int(batch._workspace.numel()), bit_equal=bool(torch.equal(out_loop, out_batch)))), flush=True)


def time_backward(a, n, r, args, kw):
    """forward-only against forward + backward on the same inputs"""
    dev = args[0].device
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    with torch.no_grad():
        for _ in range(a.warmup):
            r(*args, **kw)
        e[0].record()
        for _ in range(a.reps):
            r(*args, **kw)
        e[1].record()
    means, opac = args[0].clone().requires_grad_(True), args[2].clone().requires_grad_(True)
    leaves = dict(colors_precomp=kw["colors_precomp"].clone().requires_grad_(True), cov3D_precomp=kw["cov3D_precomp"].clone().requires_grad_(True))
    means2D = torch.zeros_like(means, requires_grad=True)
    g = torch.from_numpy(np.random.default_rng(1).uniform(-1, 1, (3, a.size, a.size)).astype(np.float32)).to(dev)
    params = [means, means2D, opac] + list(leaves.values())
    first = None
    for rep in range(a.warmup + a.reps):
        if rep == a.warmup:
            e[2].record()
        for p in params:
            p.grad = None
        img, radii = r(means, means2D, opac, **leaves)
        img.backward(g)
        if rep == 0:
            first = [p.grad.clone() for p in params]
    e[3].record()
    torch.cuda.synchronize()
    same = all(torch.equal(x, p.grad) for x, p in zip(first, params))
    print(json.dumps(dict(n=n, width=a.size, height=a.size, instances=r.last_instances, reps=a.reps, forward_ms=e[0].elapsed_time(e[1]) / a.reps,
                          forward_backward_ms=e[2].elapsed_time(e[3]) / a.reps, per_instance_buffer_bytes=36 * r.last_instances,
                          gradients_bit_equal_between_runs=bool(same), device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backward", action="store_true", help="time forward + backward of the differentiable render against the forward")
    ap.add_argument("--frames", type=int, default=0, help="time F per-frame calls against one batched call (0: the single-call timing)")
    ap.add_argument("--n", type=int, nargs="+", default=[100_000, 350_000])
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for n in a.n:
        rng = np.random.default_rng(0)
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        pos = (d * (0.5 * rng.random(n) ** (1 / 3))[:, None]).astype(np.float32)
        s2 = rng.uniform(1e-5, 4e-5, n).astype(np.float32)
        cov = np.zeros((n, 6), np.float32)
        cov[:, 0] = cov[:, 3] = cov[:, 5] = s2
        cam = look_at_camera((0.0, -2.4, 0.3), (0.0, 0.0, 0.0), 40.0, a.size, a.size, up=(0.0, 0.0, -1.0))
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        st = GaussianRasterizationSettings(a.size, a.size, cam["tanfovx"], cam["tanfovy"], t(np.ones(3, np.float32)), 1.0, t(cam["V"]), t(cam["P"]), 0,
                                           t(cam["campos"]), False, False)
        r = GaussianRasterizer(st)
        args = (t(pos), None, t(rng.uniform(0.2, 1.0, n).astype(np.float32)))
        kw = dict(colors_precomp=t(rng.uniform(0, 1, (n, 3)).astype(np.float32)), cov3D_precomp=t(cov))
        if a.backward:
            time_backward(a, n, r, args, kw)
            continue
        if a.frames > 0:
            time_frames(a, n, st, args[0], kw["cov3D_precomp"], args[2], kw["colors_precomp"])
            continue
        for _ in range(a.warmup):
            img, radii, fT, nc = r(*args, aux=True, **kw)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            r(*args, **kw)
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(n=n, width=a.size, height=a.size, instances=r.last_instances, visible=int((radii > 0).sum()),
                              call_ms=e0.elapsed_time(e1) / a.reps, reps=a.reps, mean_n_contrib=float(nc.float().mean()),
                              max_n_contrib=int(nc.max()), saturated_pixel_share=float((fT < 1e-2).float().mean()))), flush=True)


if __name__ == "__main__":
    main()
